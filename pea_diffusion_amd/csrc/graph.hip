// Graph construction: the Builder and the builders of every tape -- UNet2DConditionModel / ControlNetModel, the AutoencoderKL
// encoder and decoder, the CLIP / BERT / T5 text encoders, the CLIP vision tower and the IP-Adapter Resampler.  Each mirrors, op for op, the diffusers-0.23 /
// HF transformers graph the reference executes (train_sdxl_zh.py:397,415; restated on CPU in oracle/), with the state-dict key
// names for every weight.  Construction order is a contract: slot order is pea_unet_weight_info order, tensor order is the arena
// layout, op order is launch order.
#include <stdlib.h>

#include "model.h"

namespace {
// The UNet's upsampler convs run in their sub-pixel form (Builder::conv, ups == 2) unless PEA_UPCONV_SUBPIXEL=0 (A/B switch:
// the nearest-2x upsample folded into a 3 x 3 gather over the virtual image, 2.25 x the tap products).
static bool upconv_subpixel() {
  static const bool on = !(getenv("PEA_UPCONV_SUBPIXEL") && atoi(getenv("PEA_UPCONV_SUBPIXEL")) == 0);
  return on;
}

struct Builder {
  Tape& u;
  explicit Builder(Tape& un) : u(un) {}
  int T(long long rows, int cols, int B = 0, int H = 0, int W = 0) {
    Tn t;
    t.rows = rows; t.cols = cols; t.B = B; t.H = H; t.W = W;
    u.tn.push_back(t);
    return (int)u.tn.size() - 1;
  }
  int slot(const std::string& name, int kind, int d0, int d1, long long numel) {
    auto it = u.slot_by_name.find(name);
    if (it != u.slot_by_name.end()) return it->second;
    WSlot s;
    s.name = name; s.kind = kind; s.d0 = d0; s.d1 = d1; s.numel = numel;
    u.slots.push_back(s);
    const int id = (int)u.slots.size() - 1;
    u.slot_by_name[name] = id;
    return id;
  }
  int vec(const std::string& n, int d) { return slot(n, W_VEC, d, 0, d); }
  // N, K: stored dims; pad_mode/d/dp describe how they relate to the torch tensor (see WSlot)
  int lin(const std::string& n, int N, int K, int pad_mode = 0, int d = 0, int dp = 0) {
    int Nt = N, Kt = K;
    if (pad_mode == 1) Nt = N / dp * d;
    if (pad_mode == 2) Kt = K / dp * d;
    const int id = slot(n, W_LINEAR, Nt, Kt, (long long)Nt * Kt);
    WSlot& s = u.slots[id];
    s.st_n = N; s.st_k = K; s.pad_mode = pad_mode; s.pad_d = d; s.pad_dp = dp;
    return id;
  }
  int conv3(const std::string& n, int Co, int Ci) { return slot(n, W_CONV3, Co, Ci, 9LL * Co * Ci); }

  Op& push(int kind) {
    Op o;
    o.kind = kind;
    u.ops.push_back(o);
    return u.ops.back();
  }
  int linear(int x, const std::string& pfx, int N, bool bias, int res = -1, int pad_mode = 0, int d = 0, int dp = 0) {
    const int K = u.tn[x].cols;
    const int w = lin(pfx + ".weight", N, K, pad_mode, d, dp);
    const int b = bias ? vec(pfx + ".bias", N) : -1;
    const int out = T(u.tn[x].rows, N, u.tn[x].B, u.tn[x].H, u.tn[x].W);
    Op& o = push(OP_LINEAR);
    o.a = x; o.w = w; o.bias = b; o.out = out; o.res = res;
    return out;
  }
  // several Linear layers over the same input, stacked along N (one GEMM)
  int fused_linear(int x, const std::vector<std::string>& pfx, const std::vector<int>& Ns, bool bias,
                   const std::vector<int>* pad_d = nullptr, const std::vector<int>* pad_dp = nullptr) {
    const int K = u.tn[x].cols;
    FusedMat f;
    f.K = K; f.has_bias = bias;
    u.fused.push_back(f);
    const int fi = (int)u.fused.size() - 1;
    int off = 0;
    for (size_t i = 0; i < pfx.size(); ++i) {
      const bool padded = pad_d && (*pad_d)[i] != (*pad_dp)[i];
      const int w = padded ? lin(pfx[i] + ".weight", Ns[i], K, 1, (*pad_d)[i], (*pad_dp)[i]) : lin(pfx[i] + ".weight", Ns[i], K);
      u.slots[w].fused_parent = fi; u.slots[w].row_off = off;
      if (bias) {
        // the bias of zero-padded heads: the torch vector is heads * d long, its stored block heads * dp (pad entries zero)
        const int b = vec(pfx[i] + ".bias", padded ? Ns[i] / (*pad_dp)[i] * (*pad_d)[i] : Ns[i]);
        u.slots[b].fused_parent = fi; u.slots[b].row_off = off;
        if (padded) { u.slots[b].pad_mode = 1; u.slots[b].pad_d = (*pad_d)[i]; u.slots[b].pad_dp = (*pad_dp)[i]; }
      }
      off += Ns[i];
    }
    u.fused[fi].N = off;
    const int out = T(u.tn[x].rows, off, u.tn[x].B, u.tn[x].H, u.tn[x].W);
    Op& o = push(OP_LINEAR);
    o.a = x; o.fused = fi; o.out = out;
    return out;
  }
  int gn(int x, const std::string& pfx, bool silu, float eps) {
    const int C = u.tn[x].cols;
    const int out = T(u.tn[x].rows, C, u.tn[x].B, u.tn[x].H, u.tn[x].W);
    Op& o = push(OP_GN);
    o.a = x; o.out = out; o.w = vec(pfx + ".weight", C); o.bias = vec(pfx + ".bias", C);
    o.p0 = silu; o.f0 = eps; o.aux_bytes = sizeof(float) * 2 * u.B * u.cfg.groups;
    return out;
  }
  int ln(int x, const std::string& pfx, float eps = 1e-5f) {
    const int C = u.tn[x].cols;
    const int out = T(u.tn[x].rows, C, u.tn[x].B, u.tn[x].H, u.tn[x].W);
    Op& o = push(OP_LN);
    o.a = x; o.out = out; o.w = vec(pfx + ".weight", C); o.bias = vec(pfx + ".bias", C);
    o.f0 = eps; o.aux_bytes = sizeof(float) * 2 * u.tn[x].rows;
    return out;
  }
  int rms(int x, const std::string& name, float eps) {        // T5LayerNorm: scale only, no mean subtraction
    const int C = u.tn[x].cols;
    const int out = T(u.tn[x].rows, C, u.tn[x].B, u.tn[x].H, u.tn[x].W);
    Op& o = push(OP_LN);
    o.a = x; o.out = out; o.w = vec(name, C); o.p0 = 1; o.f0 = eps;
    return out;
  }
  int silu(int x) {
    const int out = T(u.tn[x].rows, u.tn[x].cols, u.tn[x].B, u.tn[x].H, u.tn[x].W);
    Op& o = push(OP_SILU);
    o.a = x; o.out = out;
    return out;
  }
  // ups: 1 = nearest-2x upsample folded into the 3 x 3 gather;  2 = the same conv in its sub-pixel form (four 2 x 2 kernels of
  // summed taps, one per output parity: 16 tap products per source pixel instead of 36) -- the output tensor is stored
  // depth-to-space (Tn::d2s), which only concat() and the feature taps may read
  int conv(int x, const std::string& pfx, int Cout, int stride, int ups, int rv = -1, int rv_off = 0, int res = -1) {
    const Tn& t = u.tn[x];
    const int Hv = ups ? t.H * 2 : t.H, Wv = ups ? t.W * 2 : t.W;
    const int Ho = stride == 2 ? (Hv + 1) / 2 : Hv, Wo = stride == 2 ? (Wv + 1) / 2 : Wv;
    const int w = conv3(pfx + ".weight", Cout, t.cols);
    const int b = vec(pfx + ".bias", Cout);
    const int out = T((long long)t.B * Ho * Wo, Cout, t.B, Ho, Wo);
    if (ups == 2) { u.slots[w].subpix = true; u.tn[out].d2s = true; }
    Op& o = push(OP_CONV3);
    o.a = x; o.w = w; o.bias = b; o.out = out; o.p0 = stride; o.p1 = ups; o.rv = rv; o.rv_off = rv_off; o.res = res;
    return out;
  }
  // 3x3 conv whose input tensor is stored wider than the layer's real Cin (zero-padded channels, so the implicit GEMM's
  // K = 9 * stored width stays a multiple of 64) and whose output goes into a tensor `width` >= Cout columns wide
  int conv_padded(int x, const std::string& pfx, int cin_real, int Cout, int width, int stride, int act, int res = -1) {
    const Tn t = u.tn[x];
    const int Ho = stride == 2 ? (t.H + 1) / 2 : t.H, Wo = stride == 2 ? (t.W + 1) / 2 : t.W;
    const int w = conv3(pfx + ".weight", Cout, cin_real);
    u.slots[w].pad_dp = t.cols;
    const int b = vec(pfx + ".bias", Cout);
    const int out = T((long long)t.B * Ho * Wo, width, t.B, Ho, Wo);
    u.tn[out].zero_init = width != Cout;
    Op& o = push(OP_CONV3);
    o.a = x; o.w = w; o.bias = b; o.out = out; o.p0 = stride; o.p3 = act; o.res = res;
    return out;
  }
  // AutoencoderKL pieces (diffusers 0.23 [ext]; call site train_sdxl_zh.py:306-309)
  int resnet_plain(int x, const std::string& pfx, int cout) {          // ResnetBlock2D with temb_channels=None
    const int cin = u.tn[x].cols;
    const float eps = u.cfg.eps;
    int h = gn(x, pfx + ".norm1", true, eps);
    h = conv(h, pfx + ".conv1", cout, 1, 0);
    h = gn(h, pfx + ".norm2", true, eps);
    int sc = x;
    if (cin != cout) sc = linear(x, pfx + ".conv_shortcut", cout, true);
    return conv(h, pfx + ".conv2", cout, 1, 0, -1, 0, sc);
  }
  int attention_mat(int x, const std::string& pfx) {                   // Attention(heads=1, residual_connection=True)
    const Tn t0 = u.tn[x];
    const int C = t0.cols;
    int n = gn(x, pfx + ".group_norm", false, u.cfg.eps);
    int q = linear(n, pfx + ".to_q", C, true);
    int k = linear(n, pfx + ".to_k", C, true);
    int v = linear(n, pfx + ".to_v", C, true);
    const int o = T(t0.rows, C, t0.B, t0.H, t0.W);
    {
      Op& op = push(OP_ATTN_MAT);
      op.a = q; op.b = k; op.c = v; op.out = o; op.f0 = 1.0f / sqrtf((float)C);
    }
    return linear(o, pfx + ".to_out.0", C, true, x);
  }
  // flash attention over `heads` heads of nd 64-wide slices: Q / K / V are the column blocks at qcol / kcol / vcol of tensors
  // q / k / v.  mask: Op::mask;  lse: keep the row statistics a backward pass reads (the UNet's ops)
  int attention(int q, int qcol, int k, int kcol, int v, int vcol, int heads, int Sq, int Skv, int nd, float scale, int mask = 0,
                bool lse = false) {
    const Tn t = u.tn[q];
    const int out = T(t.rows, heads * 64 * nd, t.B, t.H, t.W);
    Op& o = push(OP_ATTN);
    o.a = q; o.acol = qcol; o.b = k; o.bcol = kcol; o.c = v; o.ccol = vcol; o.out = out;
    o.p0 = heads; o.p1 = Sq; o.p2 = Skv; o.p3 = nd; o.f0 = scale; o.mask = mask;
    if (lse) o.aux_bytes = sizeof(float) * t.B * heads * Sq;
    return out;
  }
  // one pre-LN block of the CLIP towers (HF CLIPEncoderLayer keys under `p`): LN -> fused Q|K|V -> attention over all u.L tokens
  // -> out_proj + residual -> LN -> fc1 (act) -> fc2 + residual.  d / dp: head width of the checkpoint / as stored (zero padded
  // to a multiple of 64); the text tower's heads are 64 wide and it records no widths (d = dp = 0)
  int preln_block(int x, const std::string& p, int W, int heads, int d, int dp, float scale, int inter, int act, float eps, int mask) {
    const int nd = dp ? dp / 64 : 1, Cp = heads * 64 * nd;
    const std::vector<int> vd3{d, d, d}, vdp3{dp, dp, dp};
    const int n1 = ln(x, p + ".layer_norm1", eps);
    const int qkv = fused_linear(n1, {p + ".self_attn.q_proj", p + ".self_attn.k_proj", p + ".self_attn.v_proj"}, {Cp, Cp, Cp}, true,
                                 &vd3, &vdp3);
    const int att = attention(qkv, 0, qkv, Cp, qkv, 2 * Cp, heads, u.L, u.L, nd, scale, mask);
    x = linear(att, p + ".self_attn.out_proj", W, true, x, dp != d ? 2 : 0, d, dp);
    const int n2 = ln(x, p + ".layer_norm2", eps);
    const int f = linear(n2, p + ".mlp.fc1", inter, true);
    u.ops.back().p2 = act;
    return linear(f, p + ".mlp.fc2", W, true, x);
  }
  int concat(int a, int b) {
    const int out = T(u.tn[a].rows, u.tn[a].cols + u.tn[b].cols, u.tn[a].B, u.tn[a].H, u.tn[a].W);
    Op& o = push(OP_CONCAT);
    o.a = a; o.b = b; o.out = out;
    return out;
  }

  // fold the LayerNorm pushed as op `ln_idx` into the Linear pushed as op `lin_idx` (see LnFold).  Opt-in (PEA_LN_FOLD=1):
  // measured in the SDXL step (B = 4, same box, profiles/r02_ln_fold_ab.txt) the LayerNorm family drops 6.22 -> 5.28 ms but
  // the three consuming GEMMs per block pay 2.8 ms more for the heavier tile transition (s[n] quads + row statistics + one
  // more FMA per element while the matrix pipes wait), so the separate kernel stays the default.
  void fold_ln(int ln_idx, int lin_idx) {
    static const bool off = !(getenv("PEA_LN_FOLD") && atoi(getenv("PEA_LN_FOLD")) == 1);
    if (off || !(u.graph == 0 || u.graph == 2)) return;
    Op& l = u.ops[ln_idx];
    Op& g = u.ops[lin_idx];
    if (l.kind != OP_LN || g.kind != OP_LINEAR || g.a != l.out || g.res >= 0) return;
    LnFold f;
    f.ln_op = ln_idx; f.lin_op = lin_idx; f.gamma = l.w; f.beta = l.bias;
    f.K = u.tn[l.a].cols;
    if (g.fused >= 0) { f.fused = g.fused; f.N = u.fused[g.fused].N; }
    else { f.w_slot = g.w; f.bias_slot = g.bias; f.N = u.slots[g.w].st_n ? u.slots[g.w].st_n : u.slots[g.w].d0; }
    if (f.N % 16 != 0 || f.K % 64 != 0) return;
    u.folds.push_back(f);
    l.fold = g.fold = (int)u.folds.size() - 1;
  }

  int tproj_off = 0, kv_off = 0;
  int resnet(int x, const std::string& pfx, int cout) {
    const int cin = u.tn[x].cols;
    const float eps = u.cfg.eps;
    int h = gn(x, pfx + ".norm1", true, eps);
    h = conv(h, pfx + ".conv1", cout, 1, 0, u.t_tproj, tproj_off);
    tproj_off += cout;
    h = gn(h, pfx + ".norm2", true, eps);
    int sc = x;
    if (cin != cout) sc = linear(x, pfx + ".conv_shortcut", cout, true);
    return conv(h, pfx + ".conv2", cout, 1, 0, -1, 0, sc);
  }
  int transformer(int x, const std::string& pfx, int heads, int depth) {
    const int C = u.tn[x].cols;
    const Tn t0 = u.tn[x];
    const int S = t0.H * t0.W;
    const int d = C / heads, nd = (d + 63) / 64, dp = 64 * nd, Cp = heads * dp;   // heads stored dp wide (zero padded)
    const bool padded = dp != d;
    const float scale = 1.0f / sqrtf((float)d);
    const std::vector<int> vd3{d, d, d}, vdp3{dp, dp, dp};
    int h = gn(x, pfx + ".norm", false, 1e-6f);
    h = linear(h, pfx + ".proj_in", C, true);
    for (int i = 0; i < depth; ++i) {
      const std::string bp = pfx + ".transformer_blocks." + std::to_string(i);
      int n1 = ln(h, bp + ".norm1");
      const int ln1_idx = (int)u.ops.size() - 1;
      int qkv = fused_linear(n1, {bp + ".attn1.to_q", bp + ".attn1.to_k", bp + ".attn1.to_v"}, {Cp, Cp, Cp}, false, &vd3,
                             &vdp3);
      fold_ln(ln1_idx, (int)u.ops.size() - 1);
      const int a1 = attention(qkv, 0, qkv, Cp, qkv, 2 * Cp, heads, S, S, nd, scale, 0, true);
      h = linear(a1, bp + ".attn1.to_out.0", C, true, h, padded ? 2 : 0, d, dp);
      int n2 = ln(h, bp + ".norm2");
      const int ln2_idx = (int)u.ops.size() - 1;
      int q2 = linear(n2, bp + ".attn2.to_q", Cp, false, -1, padded ? 1 : 0, d, dp);
      fold_ln(ln2_idx, (int)u.ops.size() - 1);
      // K|V of every cross-attention layer come from ONE GEMM over encoder_hidden_states (u.t_kvall)
      const int kv = u.t_kvall, kvo = kv_off;
      kv_off += 2 * Cp;
      const int a2 = attention(q2, 0, kv, kvo, kv, kvo + Cp, heads, S, u.L, nd, scale, 0, true);
      h = linear(a2, bp + ".attn2.to_out.0", C, true, h, padded ? 2 : 0, d, dp);
      int n3 = ln(h, bp + ".norm3");
      const int ln3_idx = (int)u.ops.size() - 1;
      // FF projection with GEGLU fused into the GEMM epilogue: weight rows interleaved (h_i, gate_i) at load time;
      // `g` = h * gelu(gate); the [rows][8C] pre-activation (op.c) is kept only when a backward pass will need it
      int g = T(t0.rows, 4 * C, t0.B, t0.H, t0.W);
      {
        const int w = lin(bp + ".ff.net.0.proj.weight", 8 * C, C, 3, 0, 0);
        const int bsl = vec(bp + ".ff.net.0.proj.bias", 8 * C);
        u.slots[bsl].pad_mode = 3;
        const int hg = u.needs_grad ? T(t0.rows, 8 * C, t0.B, t0.H, t0.W) : -1;
        Op& o = push(OP_LINEAR);
        o.a = n3; o.w = w; o.bias = bsl; o.out = g; o.c = hg; o.p3 = 3;
      }
      fold_ln(ln3_idx, (int)u.ops.size() - 1);
      h = linear(g, bp + ".ff.net.2", C, true, h);
    }
    return linear(h, pfx + ".proj_out", C, true, x);
  }
};

// (prefix, C) of every BasicTransformerBlock in creation order (to build the stacked K|V projection)
struct CrossAttnInfo { std::string pfx; int C, heads; };
std::vector<CrossAttnInfo> enumerate_cross_attn(const PeaUnetCfg& c, bool include_up = true) {
  std::vector<CrossAttnInfo> r;
  const int n = c.n_levels;
  int cur_heads = 0;
  auto add = [&](const std::string& pfx, int C, int depth) {
    for (int k = 0; k < depth; ++k) r.push_back({pfx + ".transformer_blocks." + std::to_string(k) + ".attn2", C, cur_heads});
  };
  for (int i = 0; i < n; ++i)
    if (c.down_cross[i])
      for (int j = 0; j < c.layers_per_block; ++j) {
        cur_heads = c.heads[i];
        add("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), c.block_out[i], c.depth_down[i][j]);
      }
  cur_heads = c.heads[n - 1];
  if (c.depth_mid >= 0) add("mid_block.attentions.0", c.block_out[n - 1], c.depth_mid);
  for (int i = 0; i < n && include_up; ++i)
    if (c.up_cross[i])
      for (int j = 0; j < c.layers_per_block + 1; ++j) {
        cur_heads = c.heads[n - 1 - i];
        add("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), c.block_out[n - 1 - i],
            c.depth_up[i][j]);
      }
  return r;
}

// cout of every ResnetBlock2D in creation order (to size the fused time_emb_proj matrix)
std::vector<std::pair<std::string, int>> enumerate_resnets(const PeaUnetCfg& c, bool include_up = true) {
  std::vector<std::pair<std::string, int>> r;
  const int n = c.n_levels;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < c.layers_per_block; ++j)
      r.push_back({"down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), c.block_out[i]});
  if (c.depth_mid >= 0) {
    r.push_back({"mid_block.resnets.0", c.block_out[n - 1]});
    r.push_back({"mid_block.resnets.1", c.block_out[n - 1]});
  }
  for (int i = 0; i < n && include_up; ++i)
    for (int j = 0; j < c.layers_per_block + 1; ++j)
      r.push_back({"up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), c.block_out[n - 1 - i]});
  return r;
}
}  // namespace

// uniform per-level depths (depth[]) -> the per-position tables every builder reads
void normalize_depths(PeaUnetCfg& c) {
  if (c.per_layer_depth) return;
  const int n = c.n_levels;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      c.depth_down[i][j] = i < n ? c.depth[i] : 0;
      c.depth_up[i][j] = i < n ? c.depth[n - 1 - i] : 0;
    }
  c.depth_mid = n >= 1 ? c.depth[n - 1] : 0;
  c.per_layer_depth = 1;
}

int Tape::build_vae_encoder() {
  const PeaUnetCfg& c = cfg;
  SHAPECHK(c.n_levels >= 2 && c.n_levels <= 4, "vae: n_levels=%d", c.n_levels);
  SHAPECHK(!needs_grad && !residual_inputs, "vae encoder: inference graph only");
  SHAPECHK(c.out_channels <= 8 && c.out_channels % 2 == 0, "vae: %d moment channels", c.out_channels);
  const int f = 1 << (c.n_levels - 1);
  SHAPECHK(H % f == 0 && W % f == 0 && ((H / f) * (W / f)) % 64 == 0, "vae: image %dx%d (latent tokens must be a multiple of 64)", H, W);
  for (int i = 0; i < c.n_levels; ++i) SHAPECHK(c.block_out[i] % 64 == 0, "vae: block_out_channels[%d]=%d", i, c.block_out[i]);
  Builder bd(*this);
  int x = bd.T((long long)B * H * W, c.block_out[0], B, H, W);
  {
    Op& o = bd.push(OP_CONV_IN);
    o.out = x;
    o.w = bd.slot("encoder.conv_in.weight", W_CONV_IN, c.block_out[0], c.in_channels, 9LL * c.block_out[0] * c.in_channels);
    o.bias = bd.vec("encoder.conv_in.bias", c.block_out[0]);
  }
  const int n = c.n_levels;
  for (int i = 0; i < n; ++i) {
    const std::string p = "encoder.down_blocks." + std::to_string(i);
    for (int j = 0; j < c.layers_per_block; ++j) x = bd.resnet_plain(x, p + ".resnets." + std::to_string(j), c.block_out[i]);
    if (i != n - 1) {
      x = bd.conv(x, p + ".downsamplers.0.conv", c.block_out[i], 2, 0);
      ops.back().p2 = 1;                       // Downsample2D(padding=0): F.pad (0,1,0,1) then a stride-2 conv
    }
  }
  x = bd.resnet_plain(x, "encoder.mid_block.resnets.0", c.block_out[n - 1]);
  x = bd.attention_mat(x, "encoder.mid_block.attentions.0");
  x = bd.resnet_plain(x, "encoder.mid_block.resnets.1", c.block_out[n - 1]);
  x = bd.gn(x, "encoder.conv_norm_out", true, c.eps);
  t_out_in = x;
  {
    Op& o = bd.push(OP_CONV_OUT);
    o.a = x;
    o.w = bd.slot("encoder.conv_out.weight", W_CONV_OUT, c.out_channels, c.block_out[n - 1], 9LL * c.out_channels * c.block_out[n - 1]);
    o.bias = bd.vec("encoder.conv_out.bias", c.out_channels);
  }
  w_quant = bd.vec("quant_conv.weight", c.out_channels * c.out_channels);   // [C2][C2][1][1]
  b_quant = bd.vec("quant_conv.bias", c.out_channels);
  return PEA_OK;
}

// AutoencoderKL.decode (tests/test_sdxl_zh.py:430: `self.vae.decode(latents / scaling_factor)`): post_quant_conv (1x1,
// applied with the 1/scaling division in a pointwise kernel before the tape) -> conv_in -> mid block (resnet, single-head
// attention, resnet) -> UpDecoderBlock2D x n (layers_per_block + 1 resnets, nearest-2x + conv folded into one implicit
// GEMM) -> GroupNorm + SiLU -> conv_out.  cfg: in_channels = latent channels (4), out_channels = image channels (3),
// block_out = the ENCODER's block_out_channels (the decoder walks them reversed), H x W = LATENT size.
int Tape::build_vae_decoder() {
  const PeaUnetCfg& c = cfg;
  SHAPECHK(c.n_levels >= 2 && c.n_levels <= 4, "vae: n_levels=%d", c.n_levels);
  SHAPECHK(!needs_grad && !residual_inputs, "vae decoder: inference graph only");
  SHAPECHK(c.out_channels <= 8, "vae decoder: %d image channels", c.out_channels);
  SHAPECHK((H * W) % 64 == 0, "vae decoder: latent %dx%d (tokens must be a multiple of 64)", H, W);
  for (int i = 0; i < c.n_levels; ++i) SHAPECHK(c.block_out[i] % 64 == 0, "vae: block_out_channels[%d]=%d", i, c.block_out[i]);
  Builder bd(*this);
  const int n = c.n_levels;
  const int top = c.block_out[n - 1];
  int x = bd.T((long long)B * H * W, top, B, H, W);
  {
    Op& o = bd.push(OP_CONV_IN);
    o.out = x;
    o.w = bd.slot("decoder.conv_in.weight", W_CONV_IN, top, c.in_channels, 9LL * top * c.in_channels);
    o.bias = bd.vec("decoder.conv_in.bias", top);
  }
  x = bd.resnet_plain(x, "decoder.mid_block.resnets.0", top);
  x = bd.attention_mat(x, "decoder.mid_block.attentions.0");
  x = bd.resnet_plain(x, "decoder.mid_block.resnets.1", top);
  for (int i = 0; i < n; ++i) {
    const std::string p = "decoder.up_blocks." + std::to_string(i);
    const int co = c.block_out[n - 1 - i];
    for (int j = 0; j < c.layers_per_block + 1; ++j) x = bd.resnet_plain(x, p + ".resnets." + std::to_string(j), co);
    if (i != n - 1) x = bd.conv(x, p + ".upsamplers.0.conv", co, 1, 1);
  }
  x = bd.gn(x, "decoder.conv_norm_out", true, c.eps);
  t_out_in = x;
  {
    Op& o = bd.push(OP_CONV_OUT);
    o.a = x;
    o.w = bd.slot("decoder.conv_out.weight", W_CONV_OUT, c.out_channels, c.block_out[0], 9LL * c.out_channels * c.block_out[0]);
    o.bias = bd.vec("decoder.conv_out.bias", c.out_channels);
  }
  w_quant = bd.vec("post_quant_conv.weight", c.in_channels * c.in_channels);
  b_quant = bd.vec("post_quant_conv.bias", c.in_channels);
  return PEA_OK;
}

// Text encoders in front of the step.  flavor 0: CLIPTextModel[WithProjection] (the teacher's two
// encoders, train_sdxl_zh.py:147-150,170-285; HF transformers keys `text_model.*`, `text_projection.weight`): token +
// position embeddings, pre-LN blocks with causal attention, final LayerNorm, pooled = final[EOS] @ text_projection.
// flavor 1: BERT (the Chinese-CLIP text tower, train_sdxl_zh.py:103-107,327-329; keys `embeddings.*`,
// `encoder.layer.N.*`): word + position + token-type embeddings -> LN, post-LN blocks, key-padding mask.
int Tape::build_text() {
  const PeaTextCfg& c = tcfg;
  SHAPECHK(!needs_grad, "text encoder: inference graph only");
  if (c.flavor == 2) return build_text_t5();
  SHAPECHK(c.width % 64 == 0 && c.heads > 0 && c.width / c.heads == 64 && c.width % c.heads == 0,
           "text encoder: width %d / heads %d (head_dim must be 64)", c.width, c.heads);
  SHAPECHK(c.intermediate % 64 == 0 && c.layers >= 1 && L + c.pos_offset <= c.max_pos && c.pos_offset >= 0 && c.proj_dim % 4 == 0,
           "text encoder: dims");
  Builder bd(*this);
  const bool bert = c.flavor == 1;
  const std::string emb = bert ? "embeddings." : "text_model.embeddings.";
  const int W = c.width;
  int x = bd.T((long long)B * L, W, B, 1, L);
  {
    Op& o = bd.push(OP_EMBED);
    o.out = x;
    o.w = bd.lin(emb + (bert ? "word_embeddings.weight" : "token_embedding.weight"), c.vocab, W);
    o.bias = bd.lin(emb + (bert ? "position_embeddings.weight" : "position_embedding.weight"), c.max_pos, W);
    if (bert) o.c = bd.lin(emb + "token_type_embeddings.weight", c.pos_offset ? 1 : 2, W);   // RoBERTa family: one type row
  }
  if (bert) x = bd.ln(x, emb + "LayerNorm", c.eps);
  hidden.push_back(x);
  const float scale = 0.125f;
  for (int i = 0; i < c.layers; ++i) {
    const std::string p = (bert ? "encoder.layer." : "text_model.encoder.layers.") + std::to_string(i);
    if (bert) {
      const int qkv = bd.fused_linear(x, {p + ".attention.self.query", p + ".attention.self.key", p + ".attention.self.value"}, {W, W, W}, true);
      const int att = bd.attention(qkv, 0, qkv, W, qkv, 2 * W, c.heads, L, L, 1, scale, 2);   // key-padding mask
      int y = bd.linear(att, p + ".attention.output.dense", W, true, x);
      x = bd.ln(y, p + ".attention.output.LayerNorm", c.eps);
      int f = bd.linear(x, p + ".intermediate.dense", c.intermediate, true);
      ops.back().p2 = c.act;
      y = bd.linear(f, p + ".output.dense", W, true, x);
      x = bd.ln(y, p + ".output.LayerNorm", c.eps);
    } else {
      x = bd.preln_block(x, p, W, c.heads, 0, 0, scale, c.intermediate, c.act, c.eps, 1);   // causal
    }
    hidden.push_back(x);
  }
  t_final = x;
  if (!bert) {
    t_final = bd.ln(x, "text_model.final_layer_norm", c.eps);
    const int eos = bd.T(B, W, B);
    { Op& o = bd.push(OP_GATHER_EOS); o.a = t_final; o.out = eos; }
    t_pooled = c.proj_dim ? bd.linear(eos, "text_projection", c.proj_dim, false) : eos;
  }
  return PEA_OK;
}

// flavor 2: the T5 v1.1 encoder stack (the mT5 student option, train_sdxl_zh.py:108-112,331-345; HF transformers
// T5EncoderModel keys `shared.weight`, `encoder.block.N.layer.0.{SelfAttention.{q,k,v,o},layer_norm}`,
// `encoder.block.N.layer.1.{DenseReluDense.{wi_0,wi_1,wo},layer_norm}`, `encoder.final_layer_norm.weight`):
//   x = shared[ids];  per block:  x += o(attn(q, k, v of rms(x)))  with scores = q.k + bias[h][i][j] (no 1/sqrt(d)),
//   x += wo(gelu_new(wi_0 n) * wi_1 n), n = rms(x);  output = rms_final(x).
// The position bias comes from block 0's `relative_attention_bias` table ([buckets][heads]) through T5's bidirectional
// log-spaced buckets and is shared by all blocks; padded keys (ids == pad, right padding) are masked through kv_len.
// The gated FF runs as ONE GEMM over (wi_1_i, wi_0_i) row-interleaved weights with the h * gelu(gate) epilogue.
int Tape::build_text_t5() {
  const PeaTextCfg& c = tcfg;
  const int W = c.width, I = c.heads * 64, F = c.intermediate;
  SHAPECHK(W % 64 == 0 && c.heads > 0 && F % 64 == 0 && c.layers >= 1 && c.rel_buckets >= 2 && c.rel_buckets % 2 == 0 &&
           c.rel_max_dist > c.rel_buckets / 2, "t5 encoder: dims");
  Builder bd(*this);
  int x = bd.T((long long)B * L, W, B, 1, L);
  {
    Op& o = bd.push(OP_EMBED);
    o.out = x;
    o.w = bd.lin("shared.weight", c.vocab, W);
  }
  hidden.push_back(x);
  w_rel = bd.vec("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", c.rel_buckets * c.heads);
  for (int i = 0; i < c.layers; ++i) {
    const std::string p = "encoder.block." + std::to_string(i) + ".layer.";
    const int n1 = bd.rms(x, p + "0.layer_norm.weight", c.eps);
    const int qkv = bd.fused_linear(n1, {p + "0.SelfAttention.q", p + "0.SelfAttention.k", p + "0.SelfAttention.v"}, {I, I, I}, false);
    const int att = bd.attention(qkv, 0, qkv, I, qkv, 2 * I, c.heads, L, L, 1, 1.0f, 2 | 4);   // key padding + position bias
    x = bd.linear(att, p + "0.SelfAttention.o", W, false, x);
    const int n2 = bd.rms(x, p + "1.layer_norm.weight", c.eps);
    const int g = bd.T((long long)B * L, F, B, 1, L);
    {
      FusedMat f;
      f.K = W; f.N = 2 * F; f.has_bias = false;
      fused.push_back(f);
      const int fi = (int)fused.size() - 1;
      const int wh = bd.lin(p + "1.DenseReluDense.wi_1.weight", F, W);      // linear half -> even rows
      const int wg = bd.lin(p + "1.DenseReluDense.wi_0.weight", F, W);      // gated half  -> odd rows
      slots[wh].fused_parent = fi; slots[wh].row_off = 0; slots[wh].row_step = 2;
      slots[wg].fused_parent = fi; slots[wg].row_off = 1; slots[wg].row_step = 2;
      Op& o = bd.push(OP_LINEAR);
      o.a = n2; o.fused = fi; o.out = g; o.p3 = 3; o.p1 = 1;                // p1: gelu_new (tanh form) in the gate
    }
    x = bd.linear(g, p + "1.DenseReluDense.wo", W, false, x);
    hidden.push_back(x);
  }
  t_final = bd.rms(x, "encoder.final_layer_norm.weight", c.eps);
  return PEA_OK;
}

// CLIP vision tower (HF transformers CLIPVisionModelWithProjection; keys `vision_model.*`, `visual_projection.weight`): the image
// half of the CLIP pairs whose text half build_text() runs.  Patch rows [B*Np][Kpad] (launch_patchify: column order (c, py, px) =
// the conv weight flattened, zero-padded from 3 P P to the GEMM's K tile) -> patch GEMM (no bias) -> class row + position add +
// pre_layrnorm in one pass (launch_vision_embed) = hidden_states[0] -> pre-LN blocks with unmasked attention over Np + 1 tokens
// -> pooler_output = post_layernorm(h_N[:, 0]) -> image_embeds = pooler_output @ visual_projection^T.  Head widths 64 (ViT-B/L)
// and 80 (ViT-H/14, stored 128 wide zero-padded like the SD1.5 UNet's heads).
int Tape::build_vision() {
  const PeaVisionCfg& c = vcfg;
  SHAPECHK(!needs_grad, "vision tower: inference graph only");
  SHAPECHK(c.patch_size > 0 && c.image_size >= c.patch_size && c.image_size % c.patch_size == 0,
           "vision tower: image %d / patch %d", c.image_size, c.patch_size);
  SHAPECHK(c.heads > 0 && c.width > 0 && c.width % c.heads == 0, "vision tower: width %d / heads %d", c.width, c.heads);
  const int d = c.width / c.heads, dp = (d + 63) / 64 * 64;
  SHAPECHK(d == 64 || d == 80, "vision tower: head width %d (width %d / %d heads); 64 and 80 are supported", d, c.width, c.heads);
  SHAPECHK(c.width % 64 == 0 && c.width <= 4096 && c.intermediate > 0 && c.intermediate % 64 == 0 && c.layers >= 1 &&
           c.proj_dim > 0 && c.proj_dim % 4 == 0 && (c.act == 1 || c.act == 3), "vision tower: dims");
  const int G = c.image_size / c.patch_size, Np = G * G, K = 3 * c.patch_size * c.patch_size, Kpad = (K + 63) / 64 * 64;
  SHAPECHK(L == Np + 1 && B > 0, "vision tower: %d tokens for a %d x %d patch grid", L, G, G);
  Builder bd(*this);
  const int W = c.width;
  const std::string vm = "vision_model.";
  t_vrows = bd.T((long long)B * Np, Kpad, B, G, G);
  const int pe = bd.linear(t_vrows, vm + "embeddings.patch_embedding", W, false, -1, Kpad != K ? 2 : 0, K, Kpad);
  int x = bd.T((long long)B * L, W, B, 1, L);
  {
    const int cls = bd.vec(vm + "embeddings.class_embedding", W);
    const int pos = bd.lin(vm + "embeddings.position_embedding.weight", L, W);
    const int g = bd.vec(vm + "pre_layrnorm.weight", W), b = bd.vec(vm + "pre_layrnorm.bias", W);
    Op& o = bd.push(OP_VIS_EMBED);
    o.a = pe; o.out = x; o.w = cls; o.bias = pos; o.p0 = g; o.p1 = b; o.f0 = c.eps;     // (p0 / p1: weight slots, not tensors)
  }
  hidden.push_back(x);
  for (int i = 0; i < c.layers; ++i) {
    x = bd.preln_block(x, vm + "encoder.layers." + std::to_string(i), W, c.heads, d, dp, 1.0f / sqrtf((float)d), c.intermediate, c.act,
                       c.eps, 0);
    hidden.push_back(x);
  }
  t_final = x;
  const int cls = bd.T(B, W, B);
  { Op& o = bd.push(OP_CLS_ROW); o.a = x; o.out = cls; }
  t_vpool = bd.ln(cls, vm + "post_layernorm", c.eps);
  t_pooled = bd.linear(t_vpool, "visual_projection", c.proj_dim, false);
  return PEA_OK;
}

// Perceiver Resampler of the IP-Adapter "plus" files (tencent-ailab/IP-Adapter resampler.py; keys as the files hold them under
// `image_proj.`): the projection between the CLIP tower's hidden_states[-2] ([B][L][embed_dim]) and the Nq image tokens of
// cross_attention_dim that HipUNet.set_ip_tokens takes.
//   x = proj_in(hidden);  latents = `latents` repeated over the batch
//   per layer l:  xn = norm1(x), ln = norm2(latents);  q = to_q(ln);  k, v = to_kv([xn ; ln])  (L + Nq keys, ONE softmax, 1 / 8)
//                 latents += to_out(attn);  latents += ff.3(gelu(ff.1(ff.0(latents))))
//   tokens = norm_out(proj_out(latents))
// The reference concatenates xn and ln in front of to_kv.  Here to_kv runs where its rows are: one GEMM over the B L image
// rows, and -- stacked under to_q, sharing the to_kv weight slot -- one over the B Nq latent rows; OP_ATTN_FEWQ reads K1 / V1
// and K2 / V2 from the two outputs in place.  No concatenation and no copy on the tape; Q leaves its projection prescaled.
int Tape::build_resampler() {
  const PeaResamplerCfg& c = rcfg;
  SHAPECHK(!needs_grad, "resampler: inference graph only");
  SHAPECHK(c.heads > 0 && c.dim > 0 && c.dim % 64 == 0 && c.embed_dim > 0 && c.embed_dim % 64 == 0,
           "resampler: embed_dim %d / dim %d must be multiples of 64, heads %d", c.embed_dim, c.dim, c.heads);
  SHAPECHK(c.depth >= 1 && c.n_queries >= 1 && c.n_queries <= 32, "resampler: depth %d, %d queries (1..32)", c.depth, c.n_queries);
  SHAPECHK(c.ff_inner > 0 && c.ff_inner % 64 == 0 && c.out_dim > 0 && c.out_dim % 8 == 0,
           "resampler: ff_inner %d must be a multiple of 64, out_dim %d of 8", c.ff_inner, c.out_dim);
  SHAPECHK(B > 0 && L >= 1, "resampler: batch %d, %d image rows", B, L);
  Builder bd(*this);
  const int Nq = c.n_queries, I = c.heads * 64;                  // head width is 64 in every published file
  t_rs_in = bd.T((long long)B * L, c.embed_dim, B, 1, L);
  t_rs_lat = bd.T((long long)B * Nq, c.dim, B, 1, Nq);
  w_rs_lat = bd.lin("latents", Nq, c.dim);
  const int x = bd.linear(t_rs_in, "proj_in", c.dim, true);
  int lat = t_rs_lat;
  for (int l = 0; l < c.depth; ++l) {
    const std::string a = "layers." + std::to_string(l) + ".0", f = "layers." + std::to_string(l) + ".1";
    const int xn = bd.ln(x, a + ".norm1", c.eps), ln = bd.ln(lat, a + ".norm2", c.eps);
    const int qkv = bd.fused_linear(ln, {a + ".to_q", a + ".to_kv"}, {I, 2 * I}, false);      // Q | K2 | V2 over the latent rows
    const int kv = bd.linear(xn, a + ".to_kv", 2 * I, false);                                  // K1 | V1 over the image rows (same slot)
    const int att = bd.T((long long)B * Nq, I, B, 1, Nq);
    {
      Op& o = bd.push(OP_ATTN_FEWQ);
      o.a = qkv; o.acol = 0; o.k2col = I; o.v2col = 2 * I; o.b = kv; o.bcol = 0; o.c = kv; o.ccol = I; o.out = att;
      o.p0 = c.heads; o.p1 = Nq; o.p2 = L; o.p3 = 1; o.f0 = 0.125f;
    }
    lat = bd.linear(att, a + ".to_out", c.dim, false, lat);
    const int n = bd.ln(lat, f + ".0", c.eps);
    const int h = bd.linear(n, f + ".1", c.ff_inner, false);
    ops.back().p2 = 1;                                           // GELU(erf)
    lat = bd.linear(h, f + ".3", c.dim, false, lat);
  }
  const int y = bd.linear(lat, "proj_out", c.out_dim, true);
  t_final = bd.ln(y, "norm_out", c.eps);
  return PEA_OK;
}

// the attention backward takes query counts in multiples of 4 (attention.hip, launch_attention_bwd): a training context whose
// token grid breaks that (an SD1.5 mid block at a 56 x 104 latent: 7 x 13 = 91 tokens) is refused when it is created, not in its
// first backward pass
int Tape::check_attn_bwd_tokens() const {
  if (needs_grad)
    for (const Op& o : ops)
      SHAPECHK(o.kind != OP_ATTN || o.p1 % 4 == 0, "unet: latent %dx%d gives an attention over %d tokens; a training context "
               "(PEA_UNET_GRAD) needs multiples of 4", H, W, o.p1);
  return PEA_OK;
}

int Tape::build() {
  if (graph == 4) return build_text();
  if (graph == 5) return build_vision();
  if (graph == 6) return build_resampler();
  if (graph == 1) return build_vae_encoder();
  if (graph == 3) return build_vae_decoder();
  normalize_depths(cfg);
  const PeaUnetCfg& c = cfg;
  SHAPECHK(c.n_levels >= 2 && c.n_levels <= 4, "unet: n_levels=%d", c.n_levels);
  SHAPECHK(c.layers_per_block >= 1 && c.layers_per_block <= 3, "unet: layers_per_block=%d", c.layers_per_block);
  SHAPECHK(c.depth_mid >= 0 || graph == 0, "controlnet: a mid block is required");
  for (int i = 0; i < c.n_levels; ++i) {
    SHAPECHK(c.block_out[i] % 64 == 0, "unet: block_out_channels[%d]=%d must be a multiple of 64", i, c.block_out[i]);
    if (c.down_cross[i] || c.up_cross[c.n_levels - 1 - i] || i == c.n_levels - 1)
      SHAPECHK(c.heads[i] > 0 && c.block_out[i] % c.heads[i] == 0 && c.block_out[i] / c.heads[i] <= 192 &&
                   (c.block_out[i] / c.heads[i]) % 8 == 0,
               "unet: level %d has %d heads over %d channels; head_dim must be a multiple of 8 and <= 192", i,
               c.heads[i], c.block_out[i]);
  }
  if (inpaint_inputs) {
    SHAPECHK(graph == 0 && !needs_grad, "unet: PEA_UNET_INPAINT_INPUTS is an inference flag (not with PEA_UNET_GRAD)");
    SHAPECHK(c.in_channels == 2 * c.out_channels + 1, "unet: PEA_UNET_INPAINT_INPUTS needs in_channels == 2 * out_channels + 1 "
             "(latents, mask, masked latents), got in_channels=%d out_channels=%d", c.in_channels, c.out_channels);
    SHAPECHK(W % 4 == 0, "unet: PEA_UNET_INPAINT_INPUTS needs a latent width that is a multiple of 4, got %d", W);
  }
  SHAPECHK(c.cross_dim % 64 == 0, "unet: cross_attention_dim %% 64");
  SHAPECHK((H % (1 << (c.n_levels - 1))) == 0 && (W % (1 << (c.n_levels - 1))) == 0, "unet: latent %dx%d", H, W);
  Builder bd(*this);
  const int temb_dim = c.block_out[0] * 4;
  // conditioning inputs
  t_ehs = bd.T((long long)B * L, c.cross_dim, B, 1, L);
  tn[t_ehs].rg = needs_grad;
  if (c.text_time) {
    const int pooled = c.proj_in_dim - 6 * c.add_time_dim;
    SHAPECHK(pooled > 0 && pooled % 8 == 0 && c.proj_in_dim % 64 == 0, "unet: projection dims");
    t_text = bd.T(B, pooled, B);
    tn[t_text].rg = needs_grad;
  }
  // time embedding
  int te = bd.T(B, c.block_out[0], B);
  { Op& o = bd.push(OP_TEMB); o.out = te; o.src = 0; o.p0 = c.block_out[0]; }
  if (time_cond_dim) {   // TimestepEmbedding(cond_proj_dim=...): sample + cond_proj(condition), in the GEMM's residual epilogue
    SHAPECHK(graph == 0, "unet: time_cond_proj_dim is a UNet2DConditionModel field (graph %d)", graph);
    SHAPECHK(time_cond_dim > 0 && time_cond_dim % 64 == 0,
             "unet: time_cond_proj_dim=%d must be a positive multiple of 64 (the GEMM's K tile)", time_cond_dim);
    t_tcond = bd.T(B, time_cond_dim, B);
    tn[t_tcond].zero_init = true;
    te = bd.linear(t_tcond, "time_embedding.cond_proj", c.block_out[0], false, te);
  }
  int emb = bd.linear(te, "time_embedding.linear_1", temb_dim, true);
  emb = bd.silu(emb);
  emb = bd.linear(emb, "time_embedding.linear_2", temb_dim, true);
  if (c.text_time) {
    int tid = bd.T(B, 6 * c.add_time_dim, B);
    { Op& o = bd.push(OP_TEMB); o.out = tid; o.src = 1; o.p0 = c.add_time_dim; }
    int add = bd.concat(t_text, tid);
    int a = bd.linear(add, "add_embedding.linear_1", temb_dim, true);
    a = bd.silu(a);
    emb = bd.linear(a, "add_embedding.linear_2", temb_dim, true, emb);
  }
  int semb = bd.silu(emb);
  {   // all ResnetBlock2D.time_emb_proj stacked into one GEMM over silu(emb)
    auto rs = enumerate_resnets(c, graph != 2);
    std::vector<std::string> names;
    std::vector<int> ns;
    for (auto& r : rs) { names.push_back(r.first + ".time_emb_proj"); ns.push_back(r.second); }
    t_tproj = bd.fused_linear(semb, names, ns, true);
    tproj_total = tn[t_tproj].cols;
    ops.back().p3 = 1;   // its gradient arrives through the fp32 column-sum scratch
  }
  {   // every attn2.to_k / attn2.to_v stacked into one GEMM over encoder_hidden_states
    auto ca = enumerate_cross_attn(c, graph != 2);
    std::vector<std::string> names;
    std::vector<int> ns, pd, pdp;
    for (auto& r : ca) {
      const int d = r.C / r.heads, dp = (d + 63) / 64 * 64, Cp = r.heads * dp;
      for (const char* nm : {".to_k", ".to_v"}) {
        names.push_back(r.pfx + nm); ns.push_back(Cp); pd.push_back(d); pdp.push_back(dp);
      }
    }
    t_kvall = bd.fused_linear(t_ehs, names, ns, false, &pd, &pdp);
    ops.back().p3 = 2;                      // backward: split-K dgrad (few rows, very deep K)
    kvall_total = tn[t_kvall].cols;
  }
  // conv_in
  int x = bd.T((long long)B * H * W, c.block_out[0], B, H, W);
  {
    Op& o = bd.push(OP_CONV_IN);
    o.out = x;
    o.w = bd.slot("conv_in.weight", W_CONV_IN, c.block_out[0], c.in_channels, 9LL * c.block_out[0] * c.in_channels);
    o.bias = bd.vec("conv_in.bias", c.block_out[0]);
  }
  if (graph == 2) {
    // ControlNetConditioningEmbedding (diffusers 0.23 [ext]; call site tests/test_sdxl_zh_controlnet.py:510-519):
    // conv_in 3->16 + SiLU, then (16->16, 16->32 /2, 32->32, 32->96 /2, 96->96, 96->256 /2) each + SiLU at 8x the latent
    // resolution, then conv_out 256->block_out[0] added to conv_in(sample).  Widths are stored padded to 64 / 128.
    SHAPECHK(!needs_grad && !residual_inputs, "controlnet: inference graph only");
    SHAPECHK(c.n_levels == 3 || c.n_levels == 4, "controlnet: n_levels=%d", c.n_levels);
    const int f = cond_scale_f;
    static const int ch[4] = {16, 32, 96, 256}, wd[4] = {64, 64, 128, 256};
    ce_begin = (int)ops.size();
    int e = bd.T((long long)B * H * f * W * f, wd[0], B, H * f, W * f);
    tn[e].zero_init = true;
    {
      Op& o = bd.push(OP_CONV_IN);
      o.out = e; o.src = 1; o.p0 = ch[0]; o.p3 = 2;
      o.w = bd.slot("controlnet_cond_embedding.conv_in.weight", W_CONV_IN, ch[0], 3, 9LL * ch[0] * 3);
      o.bias = bd.vec("controlnet_cond_embedding.conv_in.bias", ch[0]);
    }
    for (int i = 0; i < 3; ++i) {
      const std::string p = "controlnet_cond_embedding.blocks.";
      e = bd.conv_padded(e, p + std::to_string(2 * i), ch[i], ch[i], wd[i], 1, 2);
      e = bd.conv_padded(e, p + std::to_string(2 * i + 1), ch[i], ch[i + 1], wd[i + 1], 2, 2);
    }
    ce_end = (int)ops.size();
    SHAPECHK(tn[e].H == H && tn[e].W == W, "controlnet: conditioning image must be 8x the latent size");
    x = bd.conv_padded(e, "controlnet_cond_embedding.conv_out", ch[3], c.block_out[0], c.block_out[0], 1, 0, x);
  }
  std::vector<int> skips{x};
  const int n = c.n_levels;
  for (int i = 0; i < n; ++i) {
    const std::string p = "down_blocks." + std::to_string(i);
    for (int j = 0; j < c.layers_per_block; ++j) {
      x = bd.resnet(x, p + ".resnets." + std::to_string(j), c.block_out[i]);
      if (c.down_cross[i]) x = bd.transformer(x, p + ".attentions." + std::to_string(j), c.heads[i], c.depth_down[i][j]);
      skips.push_back(x);
    }
    if (i != n - 1) {
      x = bd.conv(x, p + ".downsamplers.0.conv", c.block_out[i], 2, 0);
      skips.push_back(x);
    }
    taps.push_back(x);
    tap_names.push_back("d" + std::to_string(i));
  }
  auto add_external = [&](int t) {              // t + (externally supplied residual, zero until set)
    const Tn& a = tn[t];
    const int e = bd.T(a.rows, a.cols, a.B, a.H, a.W);
    const int y = bd.T(a.rows, a.cols, a.B, a.H, a.W);
    ext_res.push_back(e);
    Op& o = bd.push(OP_ADD);
    o.a = t; o.b = e; o.out = y;
    return y;
  };
  if (residual_inputs) {
    // diffusers 0.23 [ext]: the ControlNet residuals are added to the skip tensors after the down path ran, i.e.
    // only the copies the up blocks consume change (tests/test_sdxl_zh_controlnet.py:534)
    SHAPECHK(!needs_grad, "unet: residual inputs are an inference feature (no backward through them)");
    for (int& sk : skips) sk = add_external(sk);
  }
  if (c.depth_mid >= 0) {                       // mid_block_type == null (SSD-1B-style pruned UNets): no mid block at all
    x = bd.resnet(x, "mid_block.resnets.0", c.block_out[n - 1]);
    x = bd.transformer(x, "mid_block.attentions.0", c.heads[n - 1], c.depth_mid);
    x = bd.resnet(x, "mid_block.resnets.1", c.block_out[n - 1]);
    taps.push_back(x);
    tap_names.push_back("m");
  }
  if (residual_inputs) x = add_external(x);     // mid_block_additional_residual (:535)
  if (graph == 2) {
    // zero-convs: one 1x1 conv per skip tensor and one for the mid block; their outputs ARE the residuals
    for (size_t k = 0; k < skips.size(); ++k)
      cn_out.push_back(bd.linear(skips[k], "controlnet_down_blocks." + std::to_string(k), tn[skips[k]].cols, true));
    cn_out.push_back(bd.linear(x, "controlnet_mid_block", tn[x].cols, true));
    SHAPECHK(bd.kv_off == kvall_total, "controlnet: stacked K|V projection layout mismatch (%d vs %d)", bd.kv_off, kvall_total);
    return check_attn_bwd_tokens();
  }
  for (int i = 0; i < n; ++i) {
    const std::string p = "up_blocks." + std::to_string(i);
    const int lvl = n - 1 - i;
    for (int j = 0; j < c.layers_per_block + 1; ++j) {
      const int sk = skips.back();
      skips.pop_back();
      x = bd.concat(x, sk);
      ops.back().p0 = i + 1;                       // FreeU's tag (Tape::set_freeu): the up block of this concat, plus one
      x = bd.resnet(x, p + ".resnets." + std::to_string(j), c.block_out[lvl]);
      if (c.up_cross[i]) x = bd.transformer(x, p + ".attentions." + std::to_string(j), c.heads[lvl], c.depth_up[i][j]);
    }
    if (i != n - 1) x = bd.conv(x, p + ".upsamplers.0.conv", c.block_out[lvl], 1, upconv_subpixel() ? 2 : 1);
    taps.push_back(x);
    tap_names.push_back("u" + std::to_string(i));
  }
  SHAPECHK(skips.empty(), "unet: skip stack not consumed (%d left)", (int)skips.size());
  SHAPECHK(bd.kv_off == kvall_total, "unet: stacked K|V projection layout mismatch (%d vs %d)", bd.kv_off, kvall_total);
  x = bd.gn(x, "conv_norm_out", true, c.eps);
  t_out_in = x;
  {
    Op& o = bd.push(OP_CONV_OUT);
    o.a = x;
    o.w = bd.slot("conv_out.weight", W_CONV_OUT, c.out_channels, c.block_out[0], 9LL * c.out_channels * c.block_out[0]);
    o.bias = bd.vec("conv_out.bias", c.out_channels);
  }
  // requires-grad propagation + which weights need a dgrad layout
  for (Op& o : ops) {
    bool rg = false;
    for (int t : {o.a, o.b, o.kind == OP_LINEAR ? -1 : o.c, o.res, o.rv})
      if (t >= 0 && tn[t].rg) rg = true;
    if (o.out >= 0) tn[o.out].rg = tn[o.out].rg || rg;
    if ((o.kind == OP_LINEAR || o.kind == OP_CONV3) && o.a >= 0 && tn[o.a].rg) {
      if (o.fused >= 0) fused[o.fused].need_wt = true;
      else slots[o.w].need_wt = true;
    }
  }
  return check_attn_bwd_tokens();
}

// Every flash-attention op takes its Q from the projection right in front of it (fused Q|K|V: columns [0, C); to_q: the
// whole output) and nothing else reads that block: the projection's epilogue multiplies it by softmax_scale * log2(e)
// (GemmP::qscale: one rounding, from the fp32 accumulator) and the attention kernels run in the log2 domain without a
// per-score multiply (AttnP::q_prescaled).  The attention backward returns the gradient w.r.t. the unscaled q, so the
// projection's data-gradient GEMM is unchanged.
void Tape::tag_q_prescale() {
  n_attn = n_attn_pre = 0;
  for (const Op& a : ops)
    if (is_flash_attn(a.kind)) { ++n_attn; n_attn_pre += a.pre ? 1 : 0; }
  // An attention op that fails a condition below keeps a plain Q: the kernels then round Q * scale * log2(e) to bf16 themselves
  // (attention.hip: scale_frag), one more rounding than the tagged path.  Nothing on the product's graphs may take that path
  // silently: the census (pea_tape_attention_census) is asserted by the tests for every graph, and a miss is logged once here.
  struct Census {
    Tape* t;
    ~Census() {
      t->n_attn_pre = 0;
      for (const Op& a : t->ops) t->n_attn_pre += (is_flash_attn(a.kind) && a.pre) ? 1 : 0;
      if (t->n_attn_pre != t->n_attn && !t->plan_only)
        fprintf(stderr, "pea: graph %d: %d of %d attention ops run on a plain (not prescaled) Q\n", t->graph,
                t->n_attn - t->n_attn_pre, t->n_attn);
    }
  } census{this};
  for (size_t i = 0; i < ops.size(); ++i) {
    Op& a = ops[i];
    if (!is_flash_attn(a.kind) || a.pre || a.acol != 0) continue;
    int prod = -1, readers = 0;
    for (size_t j = 0; j < ops.size(); ++j) {
      const Op& o = ops[j];
      if (o.out == a.a && j < i) prod = (int)j;
      if (j != i && (o.a == a.a || o.res == a.a || o.rv == a.a || (o.kind != OP_LINEAR && o.kind != OP_EMBED && (o.b == a.a || o.c == a.a)))) {   // (OP_EMBED's b / c are weight slots, not tensors)
        // the attention itself may read K / V from the same tensor (fused Q|K|V): other columns, not a reader of the Q block
        ++readers;
      }
    }
    if (prod < 0 || readers) continue;
    Op& l = ops[prod];
    const int qcols = 64 * a.p3 * a.p0;                                       // heads x padded head width
    if (l.kind != OP_LINEAR || l.p2 != 0 || l.p3 == 3 || l.p3 == 2 || l.res >= 0 || l.qs_cols || qcols % 16 || qcols > tn[l.out].cols) continue;
    l.qs_cols = qcols;
    l.qs = a.f0 * 1.4426950408889634f;
    a.pre = 1;
  }
}
