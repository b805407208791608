// Training step of the score network on MI355X, under the VE, VP or sub-VP SDE (set_sde) or under the DDIM sampler's
// noise-prediction loss (set_ploss: sampler/diffusion_sampler.py:144-167).
//
// What the reference does in one step (score_sde_pytorch/losses.py:165-176): optimizer.zero_grad(); loss = loss_fn(...) (:105-134);
// loss.backward(); optimize_fn (:41-49: warm-up on state['step'], clip_grad_norm_, Adam); state['step'] += 1; ema.update
// (models/ema.py:32-49).  Here: the parameters, their gradients, both Adam moments and the EMA shadow are five flat device buffers
// in the reference's parameters() order (what the checkpoint loader and the optimizer kernels want); the forward pass walks the
// same block list as the sampling engine (NetArch::build), keeps the activations the backward pass needs and records one
// closure per operator; the backward pass runs the closures in reverse.  Every operator is one member (linear, conv3x3, group_norm,
// layer_norm, attention, add_scale) that runs its forward and pushes its backward.  Products: 3x3 convolutions forward and
// input-gradient on the engine's exact-f32 implicit-GEMM kernel (the input gradient is the same convolution on dY with flipped,
// transposed taps), everything else -- linear layers both ways, weight gradients, the attention products -- on the strided GEMM of
// train_kernels.hip.  Every gradient buffer is zero-initialised at first use and accumulated into, so fan-out (residual
// connections, U-Net skips, the shared time embedding) needs no special cases.
//
// Mixed precision (compute_dtype F16 / BF16): the residual-block convolutions run forward and data-gradient on the engine's 16-bit
// implicit GEMM (fp32 activations rounded once into a pass-local 16-bit copy, 16-bit weight copies made by prep_weights), every strided product on
// launch_tgemm16; the input and head convolutions (5 or 8 channels) keep the exact-f32 kernel for their forward and data gradient.
// The dtype is looked at in three places only: tg (which strided GEMM), conv3x3 (a convolution that has 16-bit weight copies runs on
// them) and plumbing16_ (set in build(): which form of the reduction launchers, reduce_ws hands out their workspace or
// null; the scaled backward seed; the overflow guard of apply()).  The first two are the PRODUCTS, the third is everything else the
// 16-bit step does differently; plan switch 48 (g_plan.train_plumbing16, read at build()) turns the third on in an f32 trainer, so that it
// can be held to the reference at fp32 tolerances with every product exact.
// The backward pass is seeded with S dL/do, S = 2^round(log2(B C L L)) (the fp32 seed is ~1e-5 at full size, at the bottom of
// f16's normal range; under the VP / sub-VP SDE S is chosen on the device from max|dL/do|), and S is divided out of the flat gradient buffer once at the end.  Every reduction that feeds a gradient, the
// gradient norm or an update runs in a fixed order (plumbing16_), so the gradients and the state after a 16-bit step are bitwise reproducible (the
// scalar loss itself is still summed with double atomics, shared with the fp32 step).  apply() refuses (and changes nothing) when the
// loss or the gradient norm is not finite.
#include "train.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace t2p {


static int gn_groups_of(int c) { return std::min(c / 4, 32); }   // layers.py:282

Trainer::Trainer(const t2p_model_config& mc, const t2p_train_config& tc) : mc_(mc), tc_(tc) {
  scratch_.get = [this](size_t bytes) { return pool_.get(bytes); };
  scratch_.put = [this](void* p) { pool_.put(p); };
}
Trainer::~Trainer() {}

long Trainer::poff(const std::string& name, std::vector<int64_t> shape) {
  auto it = index_.find(name);
  if (it == index_.end()) { set_last_error("trainer: no parameter " + name); return -1; }
  const TParam& p = params_[it->second];
  if (p.shape != shape) { set_last_error("trainer: unexpected shape of " + name); return -1; }
  return p.off;
}

#define T2P_OFF(dst, name, ...)                                     \
  do {                                                              \
    (dst) = poff((name), std::vector<int64_t>{__VA_ARGS__});        \
    if ((dst) < 0) return T2P_ERR_STATE;                            \
  } while (0)

int Trainer::map_layer(const Layer& l, LayerT* o) {
  o->kind = l.kind; o->in_ch = l.in_ch; o->out_ch = l.out_ch; o->up = l.up; o->down = l.down;
  const std::string& p = l.prefix;
  const int64_t ci = l.in_ch, co = l.out_ch, td = 4 * mc_.nf;
  auto norm = [&](Norm& n, const std::string& pre, int C, int G) -> int {
    T2P_OFF(n.g, pre + ".weight", C); T2P_OFF(n.b, pre + ".bias", C);
    n.C = C; n.G = G;
    return T2P_OK;
  };
  auto lin = [&](Lin& q, const std::string& w, const std::string& b, int64_t N, int64_t K, int form) -> int {   // 0 Linear, 1 conv1x1, 2 NIN
    if (form == 0) T2P_OFF(q.w, w, N, K);
    if (form == 1) T2P_OFF(q.w, w, N, K, 1, 1);
    if (form == 2) T2P_OFF(q.w, w, K, N);
    q.b = -1;
    if (!b.empty()) T2P_OFF(q.b, b, N);
    q.N = (int)N; q.K = (int)K; q.nin = form == 2;
    return T2P_OK;
  };
  auto conv = [&](Conv& c, const std::string& pre, int64_t Co, int64_t Ci) -> int {
    T2P_OFF(c.w, pre + ".weight", Co, Ci, 3, 3); T2P_OFF(c.b, pre + ".bias", Co);
    c.Co = (int)Co; c.Ci = (int)Ci; c.Cip = (int)((Ci + 7) / 8 * 8); c.Cop = (int)((Co + 7) / 8 * 8);
    return T2P_OK;
  };
  if (l.kind == 0) {
    ResL& r = o->r;
    T2P_TRY(norm(r.gn0, p + ".GroupNorm_0", (int)ci, gn_groups_of((int)ci)));
    T2P_TRY(conv(r.c0, p + ".Conv_0", co, ci));
    T2P_TRY(lin(r.dense, p + ".Dense_0.weight", p + ".Dense_0.bias", co, td, 0));
    T2P_TRY(norm(r.gn1, p + ".GroupNorm_1", (int)co, gn_groups_of((int)co)));
    T2P_TRY(conv(r.c1, p + ".Conv_1", co, co));
    r.has_sc = l.has_conv2;
    if (r.has_sc) T2P_TRY(lin(r.sc, p + ".Conv_2.weight", p + ".Conv_2.bias", co, ci, 1));
  } else if (l.kind == 1) {
    AttnL& a = o->a;
    T2P_TRY(norm(a.gn, p + ".GroupNorm_0", (int)ci, gn_groups_of((int)ci)));
    for (int i = 0; i < 4; ++i) T2P_TRY(lin(a.nin[i], p + ".NIN_" + std::to_string(i) + ".W", p + ".NIN_" + std::to_string(i) + ".b", ci, ci, 2));
  } else {
    StL& s = o->st;
    const std::string t = p + ".transformer_blocks.0";
    const int64_t c = ci, ctx = mc_.context_dim;
    T2P_TRY(norm(s.gn, p + ".norm", (int)c, 32));                         // attention.py:77: 32 groups
    T2P_TRY(lin(s.proj_in, p + ".proj_in.weight", p + ".proj_in.bias", c, c, 1));
    T2P_TRY(lin(s.q1, t + ".attn1.to_q.weight", "", c, c, 0)); T2P_TRY(lin(s.k1, t + ".attn1.to_k.weight", "", c, c, 0));
    T2P_TRY(lin(s.v1, t + ".attn1.to_v.weight", "", c, c, 0)); T2P_TRY(lin(s.o1, t + ".attn1.to_out.0.weight", t + ".attn1.to_out.0.bias", c, c, 0));
    T2P_TRY(lin(s.ff1, t + ".ff.net.0.proj.weight", t + ".ff.net.0.proj.bias", 8 * c, c, 0));
    T2P_TRY(lin(s.ff2, t + ".ff.net.2.weight", t + ".ff.net.2.bias", c, 4 * c, 0));
    T2P_TRY(lin(s.q2, t + ".attn2.to_q.weight", "", c, c, 0)); T2P_TRY(lin(s.k2, t + ".attn2.to_k.weight", "", c, ctx, 0));
    T2P_TRY(lin(s.v2, t + ".attn2.to_v.weight", "", c, ctx, 0)); T2P_TRY(lin(s.o2, t + ".attn2.to_out.0.weight", t + ".attn2.to_out.0.bias", c, c, 0));
    for (int i = 0; i < 3; ++i) T2P_TRY(norm(s.ln[i], t + ".norm" + std::to_string(i + 1), (int)c, 1));
    T2P_TRY(lin(s.proj_out, p + ".proj_out.weight", p + ".proj_out.bias", c, c, 1));
  }
  return T2P_OK;
}

int Trainer::build() {
  T2P_REQUIRE(mc_.compute_dtype == DT_F32 || mc_.compute_dtype == DT_F16 || mc_.compute_dtype == DT_BF16,
              "the training step computes in f32, f16 or bf16");
  dt_ = mc_.compute_dtype;
  plumbing16_ = dt_ != DT_F32 || g_plan.train_plumbing16;   // which products (dt_) and which plumbing are two questions; with it every
                                                       // reduction runs in a fixed order (bitwise reproducible), without it on atomics
  T2P_REQUIRE(tc_.dropout >= 0.0 && tc_.dropout < 1.0 && tc_.ema_rate >= 0.0 && tc_.ema_rate <= 1.0, "dropout / ema_rate");
  int dev = 0;
  T2P_HIP_CHECK(hipGetDevice(&dev));       // fails without a HIP device: there is no CPU fallback
  device_ = dev;
  T2P_TRY(arch_.build(mc_));
  long off = 0;
  for (const ParamInfo& p : arch_.params) {
    TParam t;
    t.name = p.name; t.shape = p.shape; t.off = off; t.n = 1;
    for (int64_t d : p.shape) t.n *= d;
    off += t.n;
    index_[t.name] = (int)params_.size();
    params_.push_back(std::move(t));
  }
  total_ = off;
  const size_t bytes = (size_t)total_ * 4;
  P_ = (float*)pool_.persistent(bytes); Gr_ = (float*)pool_.persistent(bytes);
  M_ = (float*)pool_.persistent(bytes); V_ = (float*)pool_.persistent(bytes); E_ = (float*)pool_.persistent(bytes);
  sumsq_ = (double*)pool_.persistent(8); loss_dev_ = (float*)pool_.persistent(4);
  if (!P_ || !Gr_ || !M_ || !V_ || !E_ || !sumsq_ || !loss_dev_) return T2P_ERR_HIP;
  for (float* b : {P_, Gr_, M_, V_, E_}) T2P_HIP_CHECK(hipMemset(b, 0, bytes));

  const int64_t td = 4 * mc_.nf, nf = mc_.nf, ch = mc_.num_channels;
  auto top_lin = [&](Lin& q, const std::string& pre, int64_t N, int64_t K) -> int {
    T2P_OFF(q.w, pre + ".weight", N, K); T2P_OFF(q.b, pre + ".bias", N);
    q.N = (int)N; q.K = (int)K; q.nin = false;
    return T2P_OK;
  };
  T2P_TRY(top_lin(pre0_, "pre_blocks.0", td, nf));
  T2P_TRY(top_lin(pre1_, "pre_blocks.1", td, td));
  T2P_OFF(pre_conv_.w, "pre_conv.weight", nf, ch, 3, 3); T2P_OFF(pre_conv_.b, "pre_conv.bias", nf);
  pre_conv_.Co = (int)nf; pre_conv_.Ci = (int)ch; pre_conv_.Cip = 8; pre_conv_.Cop = (int)nf;
  auto map_stage = [&](const Stage& st, std::vector<LayerT>* out) -> int {
    for (const Layer& l : st.layers) {
      LayerT t;
      T2P_TRY(map_layer(l, &t));
      out->push_back(std::move(t));
    }
    return T2P_OK;
  };
  for (const Stage& st : arch_.input_stages) { in_stages_.emplace_back(); T2P_TRY(map_stage(st, &in_stages_.back())); }
  T2P_TRY(map_stage(arch_.mid_stage, &mid_));
  for (const Stage& st : arch_.out_stages) { out_stages_.emplace_back(); T2P_TRY(map_stage(st, &out_stages_.back())); }
  const int fc = arch_.final_ch;
  T2P_OFF(head_norm_.g, "out.0.weight", fc); T2P_OFF(head_norm_.b, "out.0.bias", fc);
  head_norm_.C = fc; head_norm_.G = gn_groups_of(fc);
  T2P_OFF(head_conv_.w, "out.2.weight", ch, fc, 3, 3); T2P_OFF(head_conv_.b, "out.2.bias", ch);
  head_conv_.Co = (int)ch; head_conv_.Ci = fc; head_conv_.Cip = fc; head_conv_.Cop = 8;

  // kernel-layout copies of the 3x3 convolution weights, refreshed from the flat parameters at the start of every pass
  convs_.push_back(&pre_conv_);
  auto collect = [&](std::vector<LayerT>& ls) {
    for (LayerT& l : ls)
      if (l.kind == 0) { convs_.push_back(&l.r.c0); convs_.push_back(&l.r.c1); }
  };
  for (auto& st : in_stages_) collect(st);
  collect(mid_);
  for (auto& st : out_stages_) collect(st);
  convs_.push_back(&head_conv_);
  for (Conv* c : convs_) {
    T2P_REQUIRE(c->Cip % 4 == 0 && c->Cop % 4 == 0, "convolution channel padding");
    c->wf = (float*)pool_.persistent((size_t)c->Co * 9 * c->Cip * 4);
    if (!c->wf) return T2P_ERR_HIP;
    if (c != &pre_conv_) {                      // the network input needs no gradient
      c->wd = (float*)pool_.persistent((size_t)c->Ci * 9 * c->Cop * 4);
      if (!c->wd) return T2P_ERR_HIP;
    }
    dwc_floats_ = std::max(dwc_floats_, (size_t)c->Co * 9 * c->Cip);
    if (dt_ != DT_F32 && c != &pre_conv_ && c != &head_conv_) {
      c->wf16 = pool_.persistent((size_t)c->Co * 9 * c->Cip * 2);
      c->wd16 = pool_.persistent((size_t)c->Ci * 9 * c->Cop * 2);
      if (!c->wf16 || !c->wd16) return T2P_ERR_HIP;
    }
  }
  if (plumbing16_) {
    sumsq_part_ = (double*)pool_.persistent(1024 * 8);
    if (!sumsq_part_) return T2P_ERR_HIP;
  }
  dwc_ = (float*)pool_.persistent(dwc_floats_ * 4);
  if (!dwc_) return T2P_ERR_HIP;

  std::vector<float> inv(mc_.num_scales);        // 1 / sigmas[label], sigmas descending (models/utils.py:50-60, ncsnpp.py:256-261)
  const double a = std::log(mc_.sigma_max), b = std::log(mc_.sigma_min);
  for (int i = 0; i < mc_.num_scales; ++i) inv[i] = (float)(1.0 / std::exp(a + (b - a) * (double)i / (double)(mc_.num_scales - 1)));
  inv_sigma_ = (float*)pool_.persistent(inv.size() * 4);
  if (!inv_sigma_) return T2P_ERR_HIP;
  T2P_HIP_CHECK(hipMemcpy(inv_sigma_, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
  return T2P_OK;
}

int Trainer::load_param(const char* name, const float* host, const int64_t* shape, int ndim) {
  T2P_REQUIRE(name && host && shape && ndim >= 1 && ndim <= 4, "load_param arguments");
  std::string n(name);
  if (n.rfind("module.", 0) == 0) n = n.substr(7);
  if (n == "sigmas") return T2P_OK;
  auto it = index_.find(n);
  if (it == index_.end()) return T2P_OK;            // load_state_dict(strict=False)
  const TParam& p = params_[it->second];
  T2P_REQUIRE(std::vector<int64_t>(shape, shape + ndim) == p.shape, "shape mismatch for " + n);
  T2P_HIP_CHECK(hipMemcpy(P_ + p.off, host, (size_t)p.n * 4, hipMemcpyHostToDevice));
  T2P_HIP_CHECK(hipMemcpy(E_ + p.off, host, (size_t)p.n * 4, hipMemcpyHostToDevice));   // ema.py:28-29: shadow = clone of the parameters
  return T2P_OK;
}

int Trainer::read_tensor(int which, const char* name, float* host_out) {
  T2P_REQUIRE(name && host_out && which >= 0 && which <= 4, "read_tensor arguments");
  auto it = index_.find(name);
  T2P_REQUIRE(it != index_.end(), std::string("no parameter ") + name);
  const TParam& p = params_[it->second];
  float* src[5] = {P_, Gr_, E_, M_, V_};
  T2P_HIP_CHECK(hipDeviceSynchronize());
  T2P_HIP_CHECK(hipMemcpy(host_out, src[which] + p.off, (size_t)p.n * 4, hipMemcpyDeviceToHost));
  return T2P_OK;
}
int Trainer::write_tensor(int which, const char* name, const float* host_in) {
  T2P_REQUIRE(name && host_in && which >= 0 && which <= 4, "write_tensor arguments");
  auto it = index_.find(name);
  T2P_REQUIRE(it != index_.end(), std::string("no parameter ") + name);
  const TParam& p = params_[it->second];
  float* dst[5] = {P_, Gr_, E_, M_, V_};
  T2P_HIP_CHECK(hipDeviceSynchronize());
  T2P_HIP_CHECK(hipMemcpy(dst[which] + p.off, host_in, (size_t)p.n * 4, hipMemcpyHostToDevice));
  return T2P_OK;
}
int Trainer::buffer(int which, float** device_ptr, int64_t* n) {
  T2P_REQUIRE(device_ptr && n, "train_buffer arguments");
  T2P_REQUIRE(which == 0 || which == 2, "train_buffer: which is 0 (parameters) or 2 (EMA shadow), got " + std::to_string(which));
  *device_ptr = which == 0 ? P_ : E_;
  *n = (int64_t)total_;
  return T2P_OK;
}
int Trainer::copy(int dst, int src, hipStream_t s) {
  const bool store = dst == 5 && src == 0, copy_to = dst == 0 && src == 2, restore = dst == 0 && src == 5;
  T2P_REQUIRE(store || copy_to || restore, "train_copy: the pairs are 0 -> 5 (store), 2 -> 0 (copy_to) and 5 -> 0 (restore), got " +
                                               std::to_string(src) + " -> " + std::to_string(dst));
  T2P_REQUIRE(!restore || stashed_, "train_copy: restore (5 -> 0) before any store (0 -> 5)");
  const size_t bytes = (size_t)total_ * 4;
  if (store && !stash_) {
    stash_ = (float*)pool_.persistent(bytes);
    if (!stash_) return T2P_ERR_HIP;
  }
  float* d = store ? stash_ : P_;
  const float* f = store ? P_ : (copy_to ? E_ : stash_);
  T2P_HIP_CHECK(hipMemcpyAsync(d, f, bytes, hipMemcpyDeviceToDevice, s));
  if (store) stashed_ = true;
  else T2P_TRY(prep_weights(P_, s));      // the kernel-layout and 16-bit copies of the convolution weights follow the parameters
  return T2P_OK;
}
int Trainer::set_step(int64_t step, int64_t adam_updates, int64_t ema_updates) {
  T2P_REQUIRE(step >= 0 && adam_updates >= 0 && ema_updates >= 0, "step counters");
  step_ = step; adam_k_ = adam_updates; ema_k_ = ema_updates;
  return T2P_OK;
}
int Trainer::get_step(int64_t out[3]) const { out[0] = step_; out[1] = adam_k_; out[2] = ema_k_; return T2P_OK; }
int Trainer::set_sde(int sde, double beta_min, double beta_max, const float* std_table) {
  T2P_REQUIRE(ploss_ == 0, "set_sde: this trainer has the p_loss objective (set_ploss) and keeps it");
  T2P_REQUIRE(sde == T2P_SDE_VE || sde == T2P_SDE_VP || sde == T2P_SDE_SUBVP, "set_sde: unknown SDE (T2P_SDE_VE, T2P_SDE_VP or T2P_SDE_SUBVP)");
  T2P_REQUIRE(beta_min > 0.0 && beta_max > beta_min, "set_sde: 0 < beta_min < beta_max");
  T2P_REQUIRE(sde != T2P_SDE_VP || std_table, "set_sde: the VP SDE needs sqrt_1m_alphas_cumprod (float[num_scales])");
  T2P_REQUIRE(!(sde == T2P_SDE_SUBVP && mc_.scale_by_sigma && mc_.num_scales < 1000),
              "set_sde: the sub-VP time label is 999 t: with scale_by_sigma it indexes the sigma table, which needs num_scales >= 1000");
  if (sde == T2P_SDE_VP) {
    float* tab = vp_std_ ? vp_std_ : (float*)pool_.persistent((size_t)mc_.num_scales * 4);
    if (!tab) return T2P_ERR_HIP;
    T2P_HIP_CHECK(hipDeviceSynchronize());
    T2P_HIP_CHECK(hipMemcpy(tab, std_table, (size_t)mc_.num_scales * 4, hipMemcpyHostToDevice));
    vp_std_ = tab;
  }
  sde_ = sde; beta_min_ = beta_min; beta_max_ = beta_max;
  return T2P_OK;
}
int Trainer::set_ploss(int loss_type, int timesteps, const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod) {
  T2P_REQUIRE(ploss_ == 0, "set_ploss: this trainer has the p_loss objective already and keeps it");
  T2P_REQUIRE(sde_ == T2P_SDE_VE, "set_ploss: this trainer was set to the VP or sub-VP SDE loss (set_sde) and keeps it");
  T2P_REQUIRE(loss_calls_ == 0, "set_ploss: a pass has run; the objective is chosen after create and before the first pass");
  T2P_REQUIRE(loss_type == 1 || loss_type == 2, "set_ploss: unknown loss_type (1 = l1, 2 = l2)");
  T2P_REQUIRE(timesteps >= 1 && timesteps <= (1 << 24), "set_ploss: timesteps must lie in [1, 2^24] (integer labels exact in fp32, 24-bit draws)");
  T2P_REQUIRE(!mc_.scale_by_sigma || timesteps <= mc_.num_scales,
              "set_ploss: with scale_by_sigma the network divides by sigmas[t] (ncsnpp.py:259-261): timesteps <= num_scales");
  T2P_REQUIRE(sqrt_alphas_cumprod && sqrt_one_minus_alphas_cumprod, "set_ploss: the tables sqrt_alphas_cumprod and sqrt_one_minus_alphas_cumprod (float[timesteps])");
  float* tab = (float*)pool_.persistent((size_t)timesteps * 8);
  if (!tab) return T2P_ERR_HIP;
  T2P_HIP_CHECK(hipDeviceSynchronize());
  T2P_HIP_CHECK(hipMemcpy(tab, sqrt_alphas_cumprod, (size_t)timesteps * 4, hipMemcpyHostToDevice));
  T2P_HIP_CHECK(hipMemcpy(tab + timesteps, sqrt_one_minus_alphas_cumprod, (size_t)timesteps * 4, hipMemcpyHostToDevice));
  ploss_tab_ = tab; ploss_T_ = timesteps; ploss_ = loss_type;
  return T2P_OK;
}
int Trainer::set_dropout_masks(const uint8_t* const* masks, int n) {
  T2P_REQUIRE(n == 0 || masks, "dropout masks");
  drop_masks_.assign(masks, masks + n);
  return T2P_OK;
}
int Trainer::set_ss_blocks(const int32_t* host_blocks, int n, const uint8_t* host_drop, double p) {
  T2P_REQUIRE(n >= 0 && (n == 0 || host_blocks), "set_ss_blocks arguments");
  if (n == 0) { ss_n_ = 0; return T2P_OK; }
  T2P_REQUIRE(tc_.cond_flags & 2, "set_ss_blocks: this trainer was created without the ss condition (cond_flags bit 2)");
  T2P_REQUIRE(p >= 0.0 && p <= 1.0, "set_ss_blocks: the dropout probability must lie in [0, 1]");
  int max_sample = -1;
  for (int k = 0; k < n; ++k) {
    const int32_t* b = host_blocks + 3 * k;
    T2P_REQUIRE(b[0] >= 0, "set_ss_blocks: block " + std::to_string(k) + " has a negative sample index");
    T2P_REQUIRE(b[1] >= 0 && b[2] >= 0, "set_ss_blocks: block " + std::to_string(k) + " has a negative start or end (not wrapped: the dataset never writes one)");
    max_sample = std::max(max_sample, (int)b[0]);
  }
  // no pass is in flight here (every loss / step / eval pass ends with a stream synchronisation before it returns), so the buffer is
  // free to overwrite without a device-wide wait
  if (n > ss_cap_) {                                // grows as needed; the list in it is replaced anyway
    const int cap = std::max(n, 2 * ss_cap_);
    int* nb = (int*)pool_.get((size_t)cap * 13);
    if (!nb) return T2P_ERR_HIP;
    if (ss_blocks_) pool_.put(ss_blocks_);
    ss_blocks_ = nb; ss_drop_ = (uint8_t*)(nb + 3 * (size_t)cap); ss_cap_ = cap; ss_n_ = 0;
  }
  ss_n_ = 0;                                        // a failed copy leaves no list
  T2P_HIP_CHECK(hipMemcpy(ss_blocks_, host_blocks, (size_t)n * 12, hipMemcpyHostToDevice));
  if (host_drop) T2P_HIP_CHECK(hipMemcpy(ss_drop_, host_drop, (size_t)n, hipMemcpyHostToDevice));
  ss_n_ = n; ss_max_sample_ = max_sample; ss_given_ = host_drop != nullptr; ss_p_ = p;
  return T2P_OK;
}
int check_inpaint_draw(const char* who, const int32_t* host_len_lo_hi, int B, int L, double random_p, double contiguous_p) {
  const std::string w(who);
  T2P_REQUIRE(random_p >= 0.0 && random_p <= 1.0 && contiguous_p >= 0.0 && contiguous_p <= 1.0,
              w + ": random_mask_prob and contiguous_mask_prob must lie in [0, 1]");
  T2P_REQUIRE(random_p + contiguous_p <= 1.0, w + ": random_mask_prob + contiguous_mask_prob must not exceed 1");
  for (int b = 0; b < B; ++b) {
    const int32_t l = host_len_lo_hi[3 * b], lo = host_len_lo_hi[3 * b + 1], hi = host_len_lo_hi[3 * b + 2];
    T2P_REQUIRE(l >= 0 && l <= L, w + ": sample " + std::to_string(b) + " has " + std::to_string(l) + " residues, outside [0, " + std::to_string(L) + "]");
    T2P_REQUIRE(lo >= 0 && lo < hi && hi <= l, w + ": sample " + std::to_string(b) + " (" + std::to_string(l) + " residues) has the empty or misplaced range [" +
                                                   std::to_string(lo) + ", " + std::to_string(hi) + ") for its number of masked residues (0 <= lo < hi <= l)");
  }
  return T2P_OK;
}
int Trainer::set_inpaint_draw(const int32_t* host_len_lo_hi, int B, double random_p, double contiguous_p) {
  T2P_REQUIRE(B >= 0 && (B == 0 || host_len_lo_hi), "set_inpaint_draw arguments");
  if (B == 0) { inp_n_ = 0; return T2P_OK; }
  T2P_REQUIRE(tc_.cond_flags & 4, "set_inpaint_draw: this trainer was created without the inpainting condition (cond_flags bit 4)");
  T2P_REQUIRE(mc_.max_res_num <= 256, "set_inpaint_draw: the device draw counts ranks in LDS, max_res_num <= 256");
  T2P_TRY(check_inpaint_draw("set_inpaint_draw", host_len_lo_hi, B, mc_.max_res_num, random_p, contiguous_p));
  // as set_ss_blocks: no pass is in flight here, the buffer is free to overwrite
  if (B > inp_cap_) {
    const int cap = std::max(B, 2 * inp_cap_);
    int* nb = (int*)pool_.get((size_t)cap * 12);
    if (!nb) return T2P_ERR_HIP;
    if (inp_llh_) pool_.put(inp_llh_);
    inp_llh_ = nb; inp_cap_ = cap; inp_n_ = 0;        // (the request in the old buffer goes with it)
  }
  inp_n_ = 0;                                         // a failed copy leaves no request
  T2P_HIP_CHECK(hipMemcpy(inp_llh_, host_len_lo_hi, (size_t)B * 12, hipMemcpyHostToDevice));
  inp_n_ = B; inp_p_random_ = (float)random_p; inp_contig_above_ = (float)(1.0 - contiguous_p);
  return T2P_OK;
}
int Trainer::set_context_drop(const uint8_t* host_drop, int B, double p) {
  T2P_REQUIRE(B >= 0, "set_context_drop: a negative batch size");
  if (B == 0) { ctx_n_ = 0; return T2P_OK; }
  T2P_REQUIRE(p >= 0.0 && p <= 1.0, "set_context_drop: the dropout probability must lie in [0, 1]");      // (false for a NaN)
  // as set_ss_blocks: no pass is in flight here, the buffer is free to overwrite
  if (B > ctx_cap_) {
    const int cap = std::max(B, 2 * ctx_cap_);
    uint8_t* nb = (uint8_t*)pool_.get((size_t)cap);
    if (!nb) return T2P_ERR_HIP;
    if (ctx_drop_) pool_.put(ctx_drop_);
    ctx_drop_ = nb; ctx_cap_ = cap; ctx_n_ = 0;       // (the request in the old buffer goes with it)
  }
  if (host_drop) {
    ctx_n_ = 0;                                       // a failed copy leaves no request
    T2P_HIP_CHECK(hipMemcpy(ctx_drop_, host_drop, (size_t)B, hipMemcpyHostToDevice));
  }
  ctx_n_ = B; ctx_given_ = host_drop != nullptr; ctx_p_ = p;
  return T2P_OK;
}

// ---- pass-local memory ------------------------------------------------------------------------------------------------------------------
float* Trainer::tmp(size_t bytes) {
  void* p = pool_.get(bytes);
  if (p) live_.push_back(p);
  return (float*)p;
}
TT* Trainer::act(int B, int H, int W, int C, bool needs_grad) {
  acts_.emplace_back();
  TT* t = &acts_.back();
  t->B = B; t->H = H; t->W = W; t->C = C; t->needs_grad = needs_grad;
  t->p = tmp((size_t)t->numel() * 4);
  return t->p ? t : nullptr;
}
float* Trainer::grad(TT* t) {
  if (!t->g) {
    t->g = tmp((size_t)t->numel() * 4);
    if (t->g && hipMemsetAsync(t->g, 0, (size_t)t->numel() * 4, s_) != hipSuccess) t->g = nullptr;
  }
  return t->g;
}
void Trainer::release() {
  for (void* p : live_) pool_.put(p);
  live_.clear();
  acts_.clear();
  tape_.clear();
}

#define T2P_ACT(var, ...)                    \
  TT* var = act(__VA_ARGS__);                \
  if (!var) return T2P_ERR_HIP;
#define T2P_GRAD(var, t)                     \
  float* var = grad(t);                      \
  if (!var) return T2P_ERR_HIP;

int Trainer::prep_weights(const float* P, hipStream_t s) {
  for (Conv* c : convs_) T2P_TRY(launch_conv_w_prep(P + c->w, c->wf, c->wd, c->Co, c->Ci, c->Cip, c->Cop, s));
  for (Conv* c : convs_) {
    if (!c->wf16) continue;
    T2P_TRY(launch_convert(c->wf, c->wf16, dt_, (long)c->Co * 9 * c->Cip, s));
    T2P_TRY(launch_convert(c->wd, c->wd16, dt_, (long)c->Ci * 9 * c->Cop, s));
  }
  return T2P_OK;
}

int Trainer::reduce_ws(long floats, float** ws) {
  *ws = plumbing16_ ? tmp((size_t)floats * 4) : nullptr;
  return plumbing16_ && !*ws ? T2P_ERR_HIP : T2P_OK;
}

// out [nz][N] += the column sums of the nz blocks of `rows` rows of dy: nz = 1 a bias gradient, nz = B the per-sample time-embedding bias
int train_colsum(const float* dy, int nz, long rows, int N, long ld, float* out, bool fixed_order, const ConvScratch& sc, hipStream_t s) {
  float* ws = nullptr;
  if (fixed_order) {
    ws = (float*)sc.get((size_t)colsum_ws_floats(nz, rows, N) * 4);
    if (!ws) return T2P_ERR_HIP;
  }
  const int rc = launch_colsum(dy, nz, rows, N, ld, out, N, 1, ws, s);
  if (ws) sc.put(ws);                // stream-ordered: the next user of the block runs after this reduction
  return rc;
}
int Trainer::colsum(const float* dy, int nz, long rows, int N, long ld, float* out) {
  return train_colsum(dy, nz, rows, N, ld, out, plumbing16_, scratch_, s_);
}

int train_tgemm(int dt, const TGemmArgs& a, const ConvScratch& sc, hipStream_t s) {
  if (dt == DT_F32) return launch_tgemm(a, s);
  const long n = tgemm16_ws_floats(a);
  float* ws = nullptr;
  if (n > 0) {
    ws = (float*)sc.get((size_t)n * 4);
    if (!ws) return T2P_ERR_HIP;
  }
  const int rc = launch_tgemm16(a, dt, ws, s);
  if (ws) sc.put(ws);                // stream-ordered: the next user of the block runs after this product
  return rc;
}
int Trainer::tg(const TGemmArgs& a) { return train_tgemm(dt_, a, scratch_, s_); }

// ---- operators -----------------------------------------------------------------------------------------------------------------------------
// y [B][H W][ldc] = conv3x3(x) + bias (+ bias_bn[b][:]) (+ residual_inplace, which may be y: every epilogue reads and writes an output
// element in the same thread, once -- tests/test_gpu_train_conv.py holds each plan the step takes to that), N columns written.
// w16 == nullptr: the engine's exact-f32 implicit-GEMM kernel on w; else its 16-bit kernels on w16 (the LDS-DMA implicit GEMM takes
// 16-bit A only: x is rounded once into a pass-local 16-bit copy)
int train_conv_gemm(int dt, const float* x, int B, int H, int W, int Cin, const float* w, const void* w16, long ldb, const float* bias,
                    const float* bias_bn, int N, float* y, long ldc, const float* residual_inplace, const ConvScratch& sc, hipStream_t s) {
  GemmParams p;
  p.dtype = DT_F32; p.a_f32 = 1; p.A0 = x; p.C0 = Cin; p.lda0 = Cin; p.taps = 9; p.H = H; p.W = W;
  p.Bw = w; p.ldb = ldb; p.M = B * H * W; p.N = N; p.bias_n = bias; p.bias_bn = bias_bn; p.rows_per_batch = H * W; p.ld_bn = N;
  p.R = residual_inplace; p.ldr = ldc;
  p.C = y; p.c_f32 = 1; p.ldc = ldc;
  if (!w16) return launch_gemm(p, s);
  const long n = (long)B * H * W * Cin;
  void* x16 = sc.get((size_t)n * 2);
  if (!x16) return T2P_ERR_HIP;
  p.dtype = dt; p.a_f32 = 0; p.A0 = x16; p.Bw = w16;
  int rc = launch_convert(x, x16, dt, n, s);
  if (rc == T2P_OK) rc = launch_gemm(p, s);
  sc.put(x16);                     // stream-ordered: the next user of the block runs after this convolution
  return rc;
}

// y [B][H W][Cop] = conv3x3(x [B][H W][Cip]) + bias (+ tbias[b][:]: Dense_0(act(temb)) of the block, layers.py:316); Co of the Cop
// columns are written (the head convolution: Cop = 8 > Co, the rest zero).  c.wf16 (the residual-block convolutions in 16-bit
// modes) selects the 16-bit implicit GEMM for the forward and the data gradient; the input and head convolutions keep the exact-f32 kernel
int train_conv3x3_forward(int dt, const ConvW& c, const float* x, int B, int H, int W, const float* bias, const float* tbias, float* y,
                          const ConvScratch& sc, hipStream_t s) {
  if (c.Cop != c.Co) T2P_HIP_CHECK(hipMemsetAsync(y, 0, (size_t)B * H * W * c.Cop * 4, s));
  return train_conv_gemm(dt, x, B, H, W, c.Cip, c.wf, c.wf16, 9L * c.Cip, bias, tbias, c.Co, y, c.Cop, nullptr, sc, s);
}

int train_conv3x3_backward(int dt, bool fixed_order, const ConvW& c, const float* x, const float* dy, int B, int H, int W, float* dx,
                           float* dwc, float* dw, float* dbias, float* dtbias, const ConvScratch& sc, hipStream_t s) {
  const long rows = (long)B * H * W;
  if (dx)                                          // dX = conv3x3(dY, flipped transposed taps), accumulated in place through the residual operand
    T2P_TRY(train_conv_gemm(dt, dy, B, H, W, c.Cop, c.wd, c.wd16, 9L * c.Cop, nullptr, nullptr, c.Ci, dx, c.Cip, dx, sc, s));
  T2P_HIP_CHECK(hipMemsetAsync(dwc, 0, (size_t)c.Co * 9 * c.Cip * 4, s));
  TGemmArgs w;                                     // dW[co][tap][ci] = sum_pixels dY[pixel][co] X[pixel + tap][ci]
  w.A = dy; w.sAm = 1; w.sAk = c.Cop; w.B = x; w.conv_b = 1; w.H = H; w.W = W; w.conv_C = c.Cip; w.ldx = c.Cip;
  w.C = dwc; w.ldc = 9L * c.Cip; w.M = c.Co; w.N = 9 * c.Cip; w.K = (int)rows; w.beta = 1.f; w.ksplit = 0;
  T2P_TRY(train_tgemm(dt, w, sc, s));
  T2P_TRY(launch_conv_w_grad_fold(dwc, dw, c.Co, c.Ci, c.Cip, s));
  T2P_TRY(train_colsum(dy, 1, rows, c.Co, c.Cop, dbias, fixed_order, sc, s));
  if (dtbias) T2P_TRY(train_colsum(dy, B, (long)H * W, c.Co, c.Cop, dtbias, fixed_order, sc, s));
  return T2P_OK;
}

int Trainer::conv3x3(TT* x, const Conv& c, TT* tbias, TT** out) {
  T2P_REQUIRE(x->C == c.Cip && (!tbias || (tbias->C == c.Co && c.Cop == c.Co)), "conv3x3 channels");
  T2P_ACT(y, x->B, x->H, x->W, c.Cop);
  T2P_TRY(train_conv3x3_forward(dt_, conv_w(c), x->p, x->B, x->H, x->W, Pc_ + c.b, tbias ? tbias->p : nullptr, y->p, scratch_, s_));
  *out = y;
  const Conv C = c;
  tape_.push_back([this, x, y, C, tbias]() -> int {
    if (!y->g) return T2P_OK;
    float *gx = nullptr, *gt = nullptr;
    if (x->needs_grad && !(gx = grad(x))) return T2P_ERR_HIP;
    if (tbias && !(gt = grad(tbias))) return T2P_ERR_HIP;
    return train_conv3x3_backward(dt_, plumbing16_, conv_w(C), x->p, y->g, x->B, x->H, x->W, gx, dwc_, Gr_ + C.w, Gr_ + C.b, gt, scratch_, s_);
  });
  return T2P_OK;
}

int Trainer::linear(TT* x, const Lin& l, TT** out) {
  T2P_REQUIRE(x->C == l.K, "linear: input width");
  T2P_ACT(y, x->B, x->H, x->W, l.N);
  const long rows = x->rows();
  T2P_REQUIRE(rows < (1L << 31), "linear: rows");
  TGemmArgs a;
  a.A = x->p; a.sAm = l.K; a.sAk = 1;
  a.B = Pc_ + l.w; a.sBk = l.nin ? l.N : 1; a.sBn = l.nin ? 1 : l.K;
  a.C = y->p; a.ldc = l.N; a.M = (int)rows; a.N = l.N; a.K = l.K;
  a.bias_n = l.b >= 0 ? Pc_ + l.b : nullptr;
  T2P_TRY(tg(a));
  *out = y;
  const Lin L = l;
  tape_.push_back([this, x, y, L, rows]() -> int {
    if (!y->g) return T2P_OK;
    if (x->needs_grad) {                         // dx += dy W
      T2P_GRAD(gx, x);
      TGemmArgs d;
      d.A = y->g; d.sAm = L.N; d.sAk = 1;
      d.B = Pc_ + L.w; d.sBk = L.nin ? 1 : L.K; d.sBn = L.nin ? L.N : 1;       // B(k = n', n = k') = W[n'][k'] (Linear) / W[k'][n'] (NIN)
      d.C = gx; d.ldc = L.K; d.M = (int)rows; d.N = L.K; d.K = L.N; d.beta = 1.f;
      T2P_TRY(tg(d));
    }
    TGemmArgs w;                                  // dW += dy^T x (Linear [N][K]) / x^T dy (NIN [K][N]); K of this product = the rows
    if (!L.nin) { w.A = y->g; w.sAm = 1; w.sAk = L.N; w.B = x->p; w.sBk = L.K; w.sBn = 1; w.M = L.N; w.N = L.K; }
    else        { w.A = x->p; w.sAm = 1; w.sAk = L.K; w.B = y->g; w.sBk = L.N; w.sBn = 1; w.M = L.K; w.N = L.N; }
    w.C = Gr_ + L.w; w.ldc = w.N; w.K = (int)rows; w.beta = 1.f; w.ksplit = 0;
    T2P_TRY(tg(w));
    if (L.b >= 0) T2P_TRY(colsum(y->g, 1, rows, L.N, L.N, Gr_ + L.b));
    return T2P_OK;
  });
  return T2P_OK;
}

int Trainer::group_norm(TT* x, const Norm& n, int silu, TT** out) {
  T2P_REQUIRE(x->C == n.C, "GroupNorm channels");
  T2P_ACT(y, x->B, x->H, x->W, x->C);
  const int B = x->B, HW = x->H * x->W;
  float* stats = tmp((size_t)B * n.G * 2 * 4);
  const int nparts = gn_num_chunks(HW) * ((n.C + 1023) / 1024);
  float* partial = tmp((size_t)B * nparts * n.G * 2 * 4);
  if (!stats || !partial) return T2P_ERR_HIP;
  GroupNormArgs a;
  a.x0 = x->p; a.C0 = n.C; a.B = B; a.HW = HW; a.G = n.G; a.eps = 1e-6f; a.partial = partial; a.stats = stats;
  T2P_TRY(launch_gn_stats(a, s_));
  GroupNormApplyArgs g;
  g.x0 = x->p; g.C0 = n.C; g.B = B; g.H = x->H; g.W = x->W; g.G = n.G; g.stats = stats; g.gamma = Pc_ + n.g; g.beta = Pc_ + n.b; g.silu = silu;
  g.out = y->p; g.dtype = DT_F32;
  T2P_TRY(launch_gn_apply(g, s_));
  *out = y;
  const Norm N = n;
  tape_.push_back([this, x, y, N, silu, stats, B, HW]() -> int {
    if (!y->g || !x->needs_grad) return T2P_OK;
    T2P_GRAD(gx, x);
    float* ws = tmp((size_t)gn_bwd_ws_floats(B, HW, N.C, N.G) * 4);
    if (!ws) return T2P_ERR_HIP;
    return launch_gn_backward(x->p, y->g, stats, Pc_ + N.g, Pc_ + N.b, silu, B, HW, N.C, N.G, gx, Gr_ + N.g, Gr_ + N.b, ws, plumbing16_, s_);
  });
  return T2P_OK;
}

int Trainer::layer_norm(TT* x, const Norm& n, TT** out) {
  T2P_REQUIRE(x->C == n.C, "LayerNorm channels");
  T2P_ACT(y, x->B, x->H, x->W, x->C);
  T2P_TRY(launch_layernorm(x->p, Pc_ + n.g, Pc_ + n.b, y->p, DT_F32, x->rows(), n.C, 1e-5f, s_));
  *out = y;
  const Norm N = n;
  tape_.push_back([this, x, y, N]() -> int {
    if (!y->g) return T2P_OK;
    T2P_GRAD(gx, x);
    float* ws = nullptr;
    T2P_TRY(reduce_ws(ln_bwd_ws_floats(x->rows(), N.C), &ws));
    return launch_ln_backward(x->p, y->g, Pc_ + N.g, x->rows(), N.C, 1e-5f, gx, Gr_ + N.g, Gr_ + N.b, ws, s_);
  });
  return T2P_OK;
}

// one operand of a product batched over (sample b, head h): element (row, col) at p[b z0 + h z1 + row s_row + col s_col]
struct HeadOp {
  float* p; long s_row, s_col, z0, z1;
  HeadOp t() const { return {p, s_col, s_row, z0, z1}; }      // the transposed view
};

// softmax(scale q k^T) v per (sample, head): q [B][nq][C], k, v [B][nk][C], head h = columns [h d, (h + 1) d)
// (CrossAttention.forward, attention.py:170-191; AttnBlockpp with one head of width C, layers.py:168-172)
int Trainer::attention(TT* q, TT* k, TT* v, int heads, float scale, TT** out) {
  const int B = q->B, nq = q->H * q->W, nk = k->H * k->W, C = q->C, d = C / heads;
  T2P_REQUIRE(k->C == C && v->C == C && C % heads == 0 && k->B == B && v->B == B && v->H * v->W == nk, "attention shapes");
  T2P_ACT(o, q->B, q->H, q->W, C);
  const size_t pbytes = (size_t)B * heads * nq * nk * 4;
  float* S = tmp(pbytes);
  float* P = tmp(pbytes);
  if (!S || !P) return T2P_ERR_HIP;
  // the two kinds of operand: an activation [B][n][C] seen per head as [n][d], and a score buffer [B][heads][nq][nk]
  auto act_op = [C, d](float* p, int n) { return HeadOp{p, C, 1, (long)n * C, d}; };
  auto score_op = [heads, nq, nk](float* p) { return HeadOp{p, nk, 1, (long)heads * nq * nk, (long)nq * nk}; };
  auto prod = [this, B, heads](const HeadOp& a, const HeadOp& b, const HeadOp& c, int M, int N, int K, float beta) -> int {   // c = a b + beta c
    TGemmArgs g;
    g.A = a.p; g.sAm = a.s_row; g.sAk = a.s_col; g.sAz0 = a.z0; g.sAz1 = a.z1;
    g.B = b.p; g.sBk = b.s_row; g.sBn = b.s_col; g.sBz0 = b.z0; g.sBz1 = b.z1;
    g.C = c.p; g.ldc = c.s_row; g.sCz0 = c.z0; g.sCz1 = c.z1;
    g.M = M; g.N = N; g.K = K; g.nz0 = B; g.nz1 = heads; g.beta = beta;
    return tg(g);
  };
  T2P_TRY(prod(act_op(q->p, nq), act_op(k->p, nk).t(), score_op(S), nq, nk, d, 0.f));           // S = q k^T
  T2P_TRY(launch_softmax(S, nk, P, nk, DT_F32, (long)B * heads * nq, nk, scale, s_));
  T2P_TRY(prod(score_op(P), act_op(v->p, nk), act_op(o->p, nq), nq, d, nk, 0.f));               // o = P v
  *out = o;
  tape_.push_back([this, q, k, v, o, P, S, B, heads, nq, nk, d, scale, act_op, score_op, prod]() -> int {
    if (!o->g) return T2P_OK;
    float* dP = S;                               // the raw scores are dead: their buffer takes dP, then dS
    T2P_TRY(prod(act_op(o->g, nq), act_op(v->p, nk).t(), score_op(dP), nq, nk, d, 0.f));        // dP = dO v^T
    if (v->needs_grad) {                         // dv += P^T dO
      T2P_GRAD(gv, v);
      T2P_TRY(prod(score_op(P).t(), act_op(o->g, nq), act_op(gv, nk), nk, d, nq, 1.f));
    }
    T2P_TRY(launch_softmax_backward(P, dP, (long)B * heads * nq, nk, scale, s_));     // dS (w.r.t. the raw scores q k^T)
    if (q->needs_grad) {                         // dq += dS k
      T2P_GRAD(gq, q);
      T2P_TRY(prod(score_op(dP), act_op(k->p, nk), act_op(gq, nq), nq, d, nk, 1.f));
    }
    if (k->needs_grad) {                         // dk += dS^T q
      T2P_GRAD(gk, k);
      T2P_TRY(prod(score_op(dP).t(), act_op(q->p, nq), act_op(gk, nk), nk, d, nq, 1.f));
    }
    return T2P_OK;
  });
  return T2P_OK;
}

int Trainer::add_scale(TT* a, TT* b, float alpha, TT** out) {
  T2P_REQUIRE(a->numel() == b->numel() && a->C == b->C, "add_scale shapes");
  T2P_ACT(y, a->B, a->H, a->W, a->C);
  T2P_TRY(launch_add_scale(a->p, b->p, alpha, y->p, y->numel(), s_));
  *out = y;
  tape_.push_back([this, a, b, y, alpha]() -> int {
    if (!y->g) return T2P_OK;
    for (TT* t : {a, b}) {
      if (!t->needs_grad) continue;
      T2P_GRAD(gt, t);
      T2P_TRY(launch_axpy(gt, y->g, alpha, y->numel(), s_));
    }
    return T2P_OK;
  });
  return T2P_OK;
}

// ResnetBlockBigGANpp.forward (layers.py:303-327); Dropout_0 is active in train mode only
int Trainer::res_block(const LayerT& L, TT* x, TT* stemb, bool train, TT** out) {
  const ResL& r = L.r;
  const int B = x->B;
  const float alpha = mc_.skip_rescale ? (float)(1.0 / std::sqrt(2.0)) : 1.f;
  TT* a0 = nullptr;
  T2P_TRY(group_norm(x, r.gn0, 1, &a0));
  TT* xs = x;
  if (L.up || L.down) {
    const bool up = L.up != 0;
    const int H2 = up ? x->H * 2 : x->H / 2, W2 = up ? x->W * 2 : x->W / 2;
    TT* src[2] = {a0, x};
    TT* dst[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
      T2P_ACT(y, B, H2, W2, x->C);
      TT* in = src[i];
      if (up) T2P_TRY(launch_up2(in->p, y->p, B, in->H, in->W, in->C, s_));
      else T2P_TRY(launch_down2(in->p, y->p, B, in->H, in->W, in->C, s_));
      tape_.push_back([this, in, y, up]() -> int {
        if (!y->g || !in->needs_grad) return T2P_OK;
        T2P_GRAD(gi, in);
        return up ? launch_up2_backward(y->g, gi, in->B, in->H, in->W, in->C, s_) : launch_down2_backward(y->g, gi, in->B, in->H, in->W, in->C, s_);
      });
      dst[i] = y;
    }
    a0 = dst[0]; xs = dst[1];
  }
  T2P_REQUIRE(r.c0.Cop == r.c0.Co && r.c1.Cop == r.c1.Co && r.c1.Cip == r.c1.Ci, "residual block channels are multiples of 8");
  TT *tb = nullptr, *h = nullptr;                  // h = Conv_0(a0) + bias + Dense_0(act(temb)) [B][Cout]
  T2P_TRY(linear(stemb, r.dense, &tb));
  T2P_TRY(conv3x3(a0, r.c0, tb, &h));
  TT* a1 = nullptr;
  T2P_TRY(group_norm(h, r.gn1, 1, &a1));
  const double drop_p = train ? tc_.dropout : 0.0; // eval mode: models/utils.py:113-115
  if (drop_p > 0.0) {                              // Dropout_0 (layers.py:318)
    const long n = a1->numel();
    const uint8_t* keep = nullptr;
    if (!drop_masks_.empty()) {
      T2P_REQUIRE(drop_index_ < (int)drop_masks_.size(), "fewer dropout masks than residual blocks");
      keep = drop_masks_[drop_index_];
    } else {
      uint8_t* m = (uint8_t*)tmp((size_t)n);
      if (!m) return T2P_ERR_HIP;
      T2P_TRY(launch_dropout_mask(m, n, (float)drop_p, tc_.seed, rng_dropout(drop_index_), s_));
      keep = m;
    }
    ++drop_index_;
    const float inv_keep = (float)(1.0 / (1.0 - drop_p));
    T2P_ACT(y, a1->B, a1->H, a1->W, a1->C);
    T2P_TRY(launch_dropout(a1->p, keep, inv_keep, y->p, n, 0, s_));
    TT* in = a1;
    tape_.push_back([this, in, y, keep, inv_keep, n]() -> int {
      if (!y->g) return T2P_OK;
      T2P_GRAD(gi, in);
      return launch_dropout(y->g, keep, inv_keep, gi, n, 1, s_);
    });
    a1 = y;
  }
  TT* h2 = nullptr;
  T2P_TRY(conv3x3(a1, r.c1, nullptr, &h2));
  TT* sc = xs;
  if (r.has_sc) T2P_TRY(linear(xs, r.sc, &sc));
  return add_scale(sc, h2, alpha, out);
}

// AttnBlockpp.forward (layers.py:160-176)
int Trainer::attn_block(const LayerT& L, TT* x, TT** out) {
  const AttnL& a = L.a;
  const float alpha = mc_.skip_rescale ? (float)(1.0 / std::sqrt(2.0)) : 1.f;
  TT *h = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *y = nullptr;
  T2P_TRY(group_norm(x, a.gn, 0, &h));
  T2P_TRY(linear(h, a.nin[0], &q));
  T2P_TRY(linear(h, a.nin[1], &k));
  T2P_TRY(linear(h, a.nin[2], &v));
  T2P_TRY(attention(q, k, v, 1, 1.f / std::sqrt((float)x->C), &o));
  T2P_TRY(linear(o, a.nin[3], &y));
  return add_scale(x, y, alpha, out);
}

// SpatialTransformer.forward with one BasicTransformerBlock (model/attention.py:208-215, 250-263)
int Trainer::st_block(const LayerT& L, TT* x, TT* ctx, TT** out) {
  const StL& s = L.st;
  const int heads = mc_.n_heads, C = x->C;
  const float scale = 1.f / std::sqrt((float)(C / heads));
  TT *a = nullptr, *t0 = nullptr;
  T2P_TRY(group_norm(x, s.gn, 0, &a));
  T2P_TRY(linear(a, s.proj_in, &t0));
  auto attn = [&](TT* t, const Norm& ln, const Lin& wq, const Lin& wk, const Lin& wv, const Lin& wo, TT* kv_src, TT** res) -> int {
    TT *l = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *y = nullptr;
    T2P_TRY(layer_norm(t, ln, &l));
    T2P_TRY(linear(l, wq, &q));
    T2P_TRY(linear(kv_src ? kv_src : l, wk, &k));
    T2P_TRY(linear(kv_src ? kv_src : l, wv, &v));
    if (kv_src && ctx_pass_n_ > 0) {
      // context dropout: to_k and to_v have no bias, so a zero context is K = V = 0 for that sample.  The row mask is applied to the
      // projections in place (no copy of the context) and, in the reverse sweep between attention's backward and the two linears', to
      // their gradients: dW_k and dW_v receive nothing from a dropped sample, as with a context that was zero
      T2P_REQUIRE(k->numel() == v->numel() && k->B == ctx_pass_n_, "context dropout: K / V shapes");
      const long n = k->numel() / k->B;
      T2P_TRY(launch_zero_sample_rows(k->p, v->p, k->B, n, ctx_drop_, s_));
      tape_.push_back([this, k, v, n]() -> int {
        float* g0 = k->g ? k->g : v->g;
        float* g1 = k->g ? v->g : nullptr;
        return g0 ? launch_zero_sample_rows(g0, g1, k->B, n, ctx_drop_, s_) : T2P_OK;
      });
    }
    T2P_TRY(attention(q, k, v, heads, scale, &o));
    T2P_TRY(linear(o, wo, &y));
    return add_scale(y, t, 1.f, res);
  };
  TT *t1 = nullptr, *t2 = nullptr;
  T2P_TRY(attn(t0, s.ln[0], s.q1, s.k1, s.v1, s.o1, nullptr, &t1));
  T2P_TRY(attn(t1, s.ln[1], s.q2, s.k2, s.v2, s.o2, ctx, &t2));
  TT *l3 = nullptr, *u = nullptr, *y = nullptr, *t3 = nullptr, *po = nullptr;
  T2P_TRY(layer_norm(t2, s.ln[2], &l3));
  T2P_TRY(linear(l3, s.ff1, &u));
  const int inner = 4 * C;
  T2P_ACT(g, u->B, u->H, u->W, inner);
  T2P_TRY(launch_geglu(u->p, g->p, DT_F32, u->rows(), inner, s_));
  tape_.push_back([this, u, g, inner]() -> int {
    if (!g->g) return T2P_OK;
    T2P_GRAD(gu, u);
    return launch_geglu_backward(u->p, g->g, gu, u->rows(), inner, s_);
  });
  T2P_TRY(linear(g, s.ff2, &y));
  T2P_TRY(add_scale(y, t2, 1.f, &t3));
  T2P_TRY(linear(t3, s.proj_out, &po));
  return add_scale(po, x, 1.f, out);
}

int Trainer::run_layers(const std::vector<LayerT>& ls, TT* h, TT* stemb, TT* ctx, bool train, TT** out) {
  for (const LayerT& l : ls) {
    TT* y = nullptr;
    if (l.kind == 0) T2P_TRY(res_block(l, h, stemb, train, &y));
    else if (l.kind == 1) T2P_TRY(attn_block(l, h, &y));
    else T2P_TRY(st_block(l, h, ctx, &y));
    h = y;
  }
  *out = h;
  return T2P_OK;
}

// loss_fn (losses.py:105-134), or p_loss (diffusion_sampler.py:150-163) after set_ploss, on the parameters P; with `backward`,
// d loss / d P accumulates into Gr_
int Trainer::forward_backward(const t2p_train_batch& b, const float* P, bool train, bool backward, float* loss_dev, float* score_out) {
  const int B = b.batch, L = mc_.max_res_num, HW = L * L, Cx = mc_.num_channels, nf = mc_.nf;
  // p_loss without a pair mask: the reference's loss as written (diffusion_sampler.py:150-163) -- every element counts, nothing is frozen
  const bool unmasked = ploss_ != 0 && !b.mask_pair;
  const int cond_flags = unmasked ? 0 : tc_.cond_flags;
  T2P_REQUIRE(b.coords_6d && (b.mask_pair || unmasked) && b.context && B > 0 && b.tokens > 0, "training batch");
  T2P_REQUIRE(!(cond_flags & 4) || b.mask_inpaint || inp_pass_n_ > 0, "the inpainting condition needs batch.mask_inpaint");
  T2P_REQUIRE(!(tc_.cond_flags & 2) || Cx >= 7, "the ss condition needs the 8-channel layout");
  Pc_ = P;
  drop_index_ = 0;
  T2P_TRY(prep_weights(P, s_));
  const long nx = (long)B * Cx * HW;
  float* t_dev = tmp(B * 4); float* stdv = tmp(B * 4); float* scale = tmp(B * 4); float* num_elem = tmp(B * 4);
  int* labels = (int*)tmp(B * 4);
  double* loss_sum = (double*)tmp(B * 8);
  float* perturbed = tmp(nx * 4);
  uint8_t* mask = (uint8_t*)tmp(nx);
  if (!t_dev || !stdv || !scale || !num_elem || !labels || !loss_sum || !perturbed || !mask) return T2P_ERR_HIP;
  // per sample: the std of the loss, the mean coefficient (VP / sub-VP), the time label and the signed scale that turns the network's
  // output into the score (VE: 1 or 1 / sigma; VP: -1 / std_table[label]; sub-VP: -1 / std; models/utils.py:138-171)
  float* mean_coef = nullptr; float* labels_f = nullptr;
  if (ploss_) {                                   // the integer timestep, its two table entries, the integer label
    mean_coef = tmp(B * 4);
    if (!mean_coef) return T2P_ERR_HIP;
    T2P_TRY(launch_ploss_prepare(b.t, B, ploss_T_, ploss_tab_, ploss_tab_ + ploss_T_, mc_.scale_by_sigma ? inv_sigma_ : nullptr, mc_.num_scales,
                                 tc_.seed, rng_ploss_t(), t_dev, mean_coef, stdv, labels, scale, s_));
  } else if (sde_ == T2P_SDE_VE) {
    T2P_TRY(launch_dsm_prepare(b.t, B, (float)tc_.t_eps, (float)mc_.sigma_min, (float)mc_.sigma_max, mc_.num_scales,
                               mc_.scale_by_sigma ? inv_sigma_ : nullptr, tc_.seed, rng_t(), t_dev, stdv, labels, scale, s_));
  } else {
    mean_coef = tmp(B * 4); labels_f = tmp(B * 4);
    if (!mean_coef || !labels_f) return T2P_ERR_HIP;
    T2P_TRY(launch_dsm_prepare_vp(b.t, B, (float)tc_.t_eps, beta_min_, beta_max_, sde_ == T2P_SDE_SUBVP, mc_.num_scales, vp_std_,
                                  mc_.scale_by_sigma ? inv_sigma_ : nullptr, tc_.seed, rng_t(), t_dev, mean_coef, stdv,
                                  labels, labels_f, scale, s_));
  }
  const float* z = b.z;
  if (!z) {
    float* zb = tmp(nx * 4);
    if (!zb) return T2P_ERR_HIP;
    T2P_TRY(launch_philox_normal(zb, nx, tc_.seed, rng_z(), nullptr, s_));
    z = zb;
  }
  // block_dropout (losses.py:54-64, :106-107): the dropped blocks as residue flags; coords_6d itself stays as the caller gave it
  uint8_t* ss_rows = nullptr;
  if (ss_pass_n_ > 0) {
    ss_rows = (uint8_t*)tmp((size_t)B * L);
    if (!ss_rows) return T2P_ERR_HIP;
    T2P_TRY(launch_ss_block_rows(ss_blocks_, ss_pass_n_, ss_given_ ? ss_drop_ : nullptr, (float)ss_p_, tc_.seed, rng_ss(), B, L, ss_rows,
                                 nullptr, s_));
  }
  // random_mask_batch (utils.py:15-60; train.py:176, :193): a batch without mask_inpaint and a request for this pass -- the mask is drawn
  // here and goes where batch.mask_inpaint goes
  const uint8_t* mask_inpaint = unmasked ? nullptr : b.mask_inpaint;
  const uint8_t* mask_pair = b.mask_pair;
  if (unmasked) {
    uint8_t* ones = (uint8_t*)tmp((size_t)B * HW);
    if (!ones) return T2P_ERR_HIP;
    T2P_HIP_CHECK(hipMemsetAsync(ones, 1, (size_t)B * HW, s_));
    mask_pair = ones;
  }
  if (inp_pass_n_ > 0) {
    uint8_t* drawn = (uint8_t*)tmp((size_t)B * L + (size_t)B * HW);      // [B][L] residue flags, then the [B][L][L] pair mask
    if (!drawn) return T2P_ERR_HIP;
    T2P_TRY(launch_inpaint_mask_draw(inp_llh_, B, L, inp_p_random_, inp_contig_above_, tc_.seed, rng_inpaint(), -1, drawn, drawn + (size_t)B * L,
                                     nullptr, s_));
    mask_inpaint = drawn + (size_t)B * L;
  }
  T2P_TRY(launch_dsm_perturb(b.coords_6d, z, stdv, mean_coef, mask_pair, mask_inpaint, cond_flags, B, Cx, L, perturbed, mask, num_elem, s_,
                             ss_rows));
  // text-context dropout: the decisions of this pass, drawn here unless they were given.  batch.context itself stays as the caller gave
  // it; every cross-attention zeroes the dropped samples' rows of its projected K and V (st_block)
  if (ctx_pass_n_ > 0 && !ctx_given_) T2P_TRY(launch_context_drop_draw(B, (float)ctx_p_, tc_.seed, rng_ctx(), ctx_drop_, s_));

  // UNetModel.forward (ncsnpp.py:220-263)
  T2P_ACT(x0, B, L, L, 8, false);
  T2P_TRY(launch_nchw_to_nhwc(perturbed, x0->p, B, Cx, HW, 8, s_));
  T2P_ACT(emb, B, 1, 1, nf, false);
  T2P_TRY(launch_timestep_embedding(labels, labels_f, nullptr, emb->p, B, nf, s_));   // VP / sub-VP: the fractional label; p_loss: the integer
  TT *te1 = nullptr, *temb = nullptr;
  T2P_TRY(linear(emb, pre0_, &te1));
  T2P_TRY(linear(te1, pre1_, &temb));
  T2P_ACT(stemb, B, 1, 1, temb->C);                // act(temb): the same tensor for every block (layers.py:316)
  T2P_TRY(launch_silu(temb->p, stemb->p, temb->numel(), s_));
  tape_.push_back([this, temb, stemb]() -> int {
    if (!stemb->g) return T2P_OK;
    T2P_GRAD(gt, temb);
    return launch_silu_backward(temb->p, stemb->g, gt, temb->numel(), s_);
  });
  acts_.emplace_back();                            // the text context: caller-owned, no gradient
  TT* ctx = &acts_.back();
  ctx->p = const_cast<float*>(b.context); ctx->B = B; ctx->H = b.tokens; ctx->W = 1; ctx->C = mc_.context_dim; ctx->needs_grad = false;

  TT* h0 = nullptr;
  T2P_TRY(conv3x3(x0, pre_conv_, nullptr, &h0));   // x0 needs no gradient: weight and bias gradients only
  std::vector<TT*> hs{h0};
  TT* h = h0;
  for (const auto& st : in_stages_) {
    T2P_TRY(run_layers(st, h, stemb, ctx, train, &h));
    hs.push_back(h);
  }
  T2P_TRY(run_layers(mid_, h, stemb, ctx, train, &h));
  for (const auto& st : out_stages_) {
    TT* skip = hs.back();
    hs.pop_back();
    T2P_REQUIRE(skip->H == h->H && skip->B == h->B, "skip stack mismatch");
    T2P_ACT(cat, B, h->H, h->W, h->C + skip->C);   // torch.cat([h, hs.pop()], dim=1), ncsnpp.py:250
    T2P_TRY(launch_copy_cols(h->p, h->C, 0, cat->p, cat->C, 0, h->rows(), h->C, 0, s_));
    T2P_TRY(launch_copy_cols(skip->p, skip->C, 0, cat->p, cat->C, h->C, h->rows(), skip->C, 0, s_));
    TT* hin = h;
    tape_.push_back([this, hin, skip, cat]() -> int {
      if (!cat->g) return T2P_OK;
      T2P_GRAD(g0, hin);
      T2P_GRAD(g1, skip);
      T2P_TRY(launch_copy_cols(cat->g, cat->C, 0, g0, hin->C, 0, hin->rows(), hin->C, 1, s_));
      return launch_copy_cols(cat->g, cat->C, hin->C, g1, skip->C, 0, hin->rows(), skip->C, 1, s_);
    });
    T2P_TRY(run_layers(st, cat, stemb, ctx, train, &h));
  }
  T2P_REQUIRE(hs.empty(), "skip stack not consumed");
  TT* a = nullptr;
  T2P_TRY(group_norm(h, head_norm_, 1, &a));
  TT* o = nullptr;                                 // head convolution: Cx of its 8 columns used, the rest zero
  T2P_TRY(conv3x3(a, head_conv_, nullptr, &o));
  float* d_o = nullptr;
  if (backward) {
    d_o = grad(o);
    if (!d_o) return T2P_ERR_HIP;
  }
  if (ploss_) T2P_TRY(launch_ploss_loss(ploss_ == 1, o->p, 8, z, scale, mask, num_elem, B, Cx, L, loss_sum, d_o, 8, score_out, s_));
  else T2P_TRY(launch_dsm_loss(o->p, 8, z, stdv, scale, mask, num_elem, B, Cx, L, loss_sum, d_o, 8, score_out, s_));
  T2P_TRY(launch_dsm_finish(loss_sum, num_elem, B, loss_dev, s_));
  // 16-bit modes: seed the backward pass with S dL/do (S a power of two: exact in fp32) and divide S out of the flat gradient buffer.
  // VE: S = 2^round(log2(B C L L)), known on the host (std / sigma[label] is about 1, so the seed is about 2 r / (num_elem B)).
  // VP / sub-VP: the seed carries std |scale| = up to 1 / sigma_min with scale_by_sigma (the sigma table is indexed by a label that
  // grows with t) and a residual r of that size, so a fixed S overflows f16 at large t: S is chosen on the device as the largest
  // power of two with S max|dL/do| <= 64, the magnitude the VE seed has.
  // p_loss: r = o / sigmas[t] - z has no std / sigma ratio that stays near 1 -- with scale_by_sigma the residual and the seed both carry
  // 1 / sigmas[t], up to 1 / sigma_min, and a fixed S overflows f16 at the last timesteps as under VP: S on the device there too; without
  // scale_by_sigma the seed is 2 r / (num_elem B) or +-1 / (num_elem B) and the VE step's host S holds.
  const bool dev_scale = backward && plumbing16_ && (sde_ != T2P_SDE_VE || (ploss_ != 0 && mc_.scale_by_sigma));
  const float S = !plumbing16_ ? 1.f : std::ldexp(1.f, (int)std::lround(std::log2((double)B * Cx * HW)));
  float* s2 = nullptr;                            // device pair {S, 1 / S} of the VP / sub-VP 16-bit step
  if (dev_scale) {
    s2 = tmp(8);
    unsigned int* amax = (unsigned int*)tmp(4);
    if (!s2 || !amax) return T2P_ERR_HIP;
    T2P_TRY(launch_seed_scale(d_o, o->numel(), 64.f, amax, s2, s_));
    T2P_TRY(launch_scale_dev(d_o, s2, o->numel(), s_));
  } else if (backward && S != 1.f) {
    T2P_TRY(launch_scale(d_o, S, o->numel(), s_));
  }
  if (backward)
    for (auto it = tape_.rbegin(); it != tape_.rend(); ++it) T2P_TRY((*it)());
  if (dev_scale) T2P_TRY(launch_scale_dev(Gr_, s2 + 1, total_, s_));
  else if (backward && S != 1.f) T2P_TRY(launch_scale(Gr_, 1.f / S, total_, s_));
  return T2P_OK;
}

int Trainer::loss(const t2p_train_batch& b, bool backward, bool use_ema, float* loss_host, float* score_out, hipStream_t s) {
  T2P_REQUIRE(loss_host, "loss output");
  ss_pass_n_ = ss_n_;                             // the block list is per-batch data: this pass consumes it, whatever becomes of the pass
  ss_n_ = 0;
  const int inp_request = inp_n_;                 // so is the random-mask request; a batch that supplies mask_inpaint ignores it
  inp_pass_n_ = b.mask_inpaint ? 0 : inp_n_;
  inp_n_ = 0;
  ctx_pass_n_ = ctx_n_;                           // and the context-dropout request
  ctx_n_ = 0;
  T2P_REQUIRE(ctx_pass_n_ == 0 || ctx_pass_n_ == b.batch,
              "context dropout: the request holds " + std::to_string(ctx_pass_n_) + " samples, the batch " + std::to_string(b.batch) +
                  "; nothing was computed or changed and the request is cleared");
  T2P_REQUIRE(inp_pass_n_ == 0 || inp_pass_n_ == b.batch,
              "inpaint draw: the request holds " + std::to_string(inp_request) + " samples, the batch " + std::to_string(b.batch) +
                  "; nothing was computed or changed and the request is cleared");
  T2P_REQUIRE(ss_pass_n_ == 0 || ss_max_sample_ < b.batch,
              "ss blocks: sample index " + std::to_string(ss_max_sample_) + " >= batch " + std::to_string(b.batch) +
                  "; nothing was computed or changed and the block list is cleared");
  T2P_REQUIRE(!(ploss_ != 0 && !b.mask_pair) || (ss_pass_n_ == 0 && inp_request == 0),
              "p_loss without mask_pair is the unmasked loss: it takes no ss block list and no inpaint draw; nothing was computed or changed "
              "and the request is cleared");
  s_ = s;
  if (backward) last_loss_finite_ = false;        // the overflow guard trusts only a completed backward pass
  if (backward) T2P_HIP_CHECK(hipMemsetAsync(Gr_, 0, (size_t)total_ * 4, s));      // optimizer.zero_grad()
  const int rc = forward_backward(b, use_ema ? E_ : P_, !use_ema, backward, loss_dev_, score_out);   // the EMA weights: eval mode
  ++loss_calls_;
  const hipError_t e = hipStreamSynchronize(s);
  release();
  if (rc != T2P_OK) return rc;
  T2P_HIP_CHECK(e);
  T2P_HIP_CHECK(hipMemcpy(loss_host, loss_dev_, 4, hipMemcpyDeviceToHost));
  if (backward) last_loss_finite_ = std::isfinite(*loss_host);
  return T2P_OK;
}

int Trainer::step(const t2p_train_batch& b, float* loss_host, hipStream_t s) {
  T2P_TRY(loss(b, true, false, loss_host, nullptr, s));
  return apply(s);
}

int Trainer::apply(hipStream_t s) {
  // optimize_fn (losses.py:41-49)
  AdamArgs a;
  a.p = P_; a.g = Gr_; a.m = M_; a.v = V_; a.n = total_;
  a.lr = (float)(tc_.warmup > 0 ? tc_.lr * std::min((double)step_ / tc_.warmup, 1.0) : tc_.lr);
  a.beta1 = (float)tc_.beta1; a.beta2 = 0.999f; a.eps = (float)tc_.eps; a.weight_decay = (float)tc_.weight_decay;
  a.one_minus_beta1 = (float)(1.0 - tc_.beta1); a.one_minus_beta2 = (float)(1.0 - 0.999);
  const int64_t k = adam_k_ + 1;
  a.bias1 = (float)(1.0 - std::pow(tc_.beta1, (double)k));
  a.bias2_sqrt = (float)std::sqrt(1.0 - std::pow(0.999, (double)k));
  a.grad_clip = (float)tc_.grad_clip;
  const bool guard = plumbing16_;                 // overflow guard (AMP's skipped step, reported): a loss or gradient norm that is not finite changes nothing
  if (guard || tc_.grad_clip >= 0) {
    if (!sumsq_part_) T2P_HIP_CHECK(hipMemsetAsync(sumsq_, 0, 8, s));     // the atomic form accumulates
    T2P_TRY(launch_sumsq(Gr_, total_, sumsq_part_, sumsq_, s));
    if (tc_.grad_clip >= 0) a.sumsq = sumsq_;
  }
  if (guard) {
    double sumsq = 0.0;
    T2P_HIP_CHECK(hipMemcpyAsync(&sumsq, sumsq_, 8, hipMemcpyDeviceToHost, s));
    T2P_HIP_CHECK(hipStreamSynchronize(s));
    T2P_REQUIRE(last_loss_finite_ && std::isfinite(sumsq),
                std::string("16-bit training step skipped: ") +
                    (last_loss_finite_ ? "the gradient norm is not finite (f16 / bf16 overflow)"
                                       : "the loss of the last backward pass is not finite (f16 / bf16 overflow), or that pass did not complete") +
                    "; parameters, optimizer state, EMA and step counters are unchanged");
  }
  T2P_TRY(launch_adam(a, s));
  adam_k_ = k;
  step_ += 1;
  // ema.update (ema.py:32-49)
  ema_k_ += 1;
  const double decay = std::min(tc_.ema_rate, (1.0 + (double)ema_k_) / (10.0 + (double)ema_k_));
  T2P_TRY(launch_ema(E_, P_, (float)(1.0 - decay), total_, s));
  T2P_HIP_CHECK(hipStreamSynchronize(s));
  return T2P_OK;
}

}  // namespace t2p
