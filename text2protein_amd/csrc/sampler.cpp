// Host side of the predictor-corrector loop (sampling.py:245-289).  One step() serves the plain and the guided loop under the VE and
// the VP SDE: guidance changes the batch of the evaluation and adds a second destination, the score itself (guidance sum, VP scale)
// is formed inside the update kernels.  No host synchronisation happens inside step(): the Langevin step size is computed on the
// device from device-side norm sums.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace t2p {

Sampler::Sampler(Engine* e, const t2p_sampler_config& cfg) : e_(e), cfg_(cfg) {}

int Sampler::init(const float* g_table_host, const int32_t* label_table_host) {
  T2P_REQUIRE(cfg_.sde == T2P_SDE_VE || cfg_.sde == T2P_SDE_VP, "the fused sampler covers the VE and VP SDEs");
  T2P_REQUIRE(cfg_.sde == T2P_SDE_VE || (g_table_host && label_table_host), "the VP SDE needs its G and label tables (t2p_sampler_create) and t2p_sampler_set_vp_tables");
  T2P_REQUIRE(cfg_.N == e_->cfg().num_scales, "sde.N must equal model.num_scales");
  T2P_REQUIRE(cfg_.batch > 0 && cfg_.global_batch >= cfg_.batch && cfg_.n_steps_each >= 1, "sampler config");
  T2P_REQUIRE(cfg_.eps >= 0.0 && cfg_.eps < 1.0, "eps must lie in [0, T)");
  const int N = cfg_.N;
  // time label of loop step i: round((T - t_i) (N - 1)) with t = linspace(T, eps, N) (sampling.py:257,
  // models/utils.py:159-171); equals i only for tiny eps, e.g. 499 of 1000 labels differ at eps = 1e-3
  std::vector<int32_t> lab(N);
  if (label_table_host) {
    std::copy(label_table_host, label_table_host + N, lab.begin());
  } else {
    for (int i = 0; i < N; ++i) {
      const double t = 1.0 + (cfg_.eps - 1.0) * (double)i / (double)(N - 1);
      lab[i] = (int32_t)std::nearbyint((1.0 - t) * (double)(N - 1));
    }
  }
  for (int i = 0; i < N; ++i) T2P_REQUIRE(lab[i] >= 0 && lab[i] < N, "time label out of range");
  std::vector<float> g(N);
  if (g_table_host) {
    std::copy(g_table_host, g_table_host + N, g.begin());
  } else {
    // VESDE.discretize (sde_lib.py:237-245): step i uses k = N-1-i on the ascending sigmas
    const double a = std::log(cfg_.sigma_min), b = std::log(cfg_.sigma_max);
    auto sig = [&](int k) { return (double)(float)std::exp(a + (b - a) * (double)k / (double)(N - 1)); };
    for (int i = 0; i < N; ++i) {
      const int k = N - 1 - i;
      const double sk = sig(k), sp = k == 0 ? 0.0 : sig(k - 1);
      g[i] = (float)std::sqrt(sk * sk - sp * sp);
    }
  }
  DevPool& pool = e_->pool();
  g_table_ = (float*)pool.persistent((size_t)N * 4);
  label_table_ = (int*)pool.persistent((size_t)N * 4);
  step_dev_ = (int*)pool.persistent(256);
  const t2p_model_config& m = e_->cfg();
  per_sample_ = (long)m.num_channels * m.max_res_num * m.max_res_num;
  n_ = per_sample_ * cfg_.batch;
  score_ = (float*)pool.persistent((size_t)n_ * 4);
  noise_ = (float*)pool.persistent((size_t)n_ * 4);
  xmean_ = (float*)pool.persistent((size_t)n_ * 4);
  sq_ws_ = (float*)pool.persistent((size_t)cfg_.batch * 64 * 2 * 4);
  sums_ = (float*)pool.persistent(256);
  if (!g_table_ || !label_table_ || !step_dev_ || !score_ || !noise_ || !xmean_ || !sq_ws_ || !sums_) return T2P_ERR_HIP;
  T2P_HIP_CHECK(hipMemcpy(g_table_, g.data(), (size_t)N * 4, hipMemcpyHostToDevice));
  T2P_HIP_CHECK(hipMemcpy(label_table_, lab.data(), (size_t)N * 4, hipMemcpyHostToDevice));
  T2P_HIP_CHECK(hipMemset(step_dev_, 0, 256));
  return T2P_OK;
}

int Sampler::reset(int step, hipStream_t s) {
  T2P_REQUIRE(step >= 0 && step < cfg_.N, "step out of range");
  T2P_HIP_CHECK(hipMemcpyAsync(step_dev_, &step, sizeof(int), hipMemcpyHostToDevice, s));
  T2P_HIP_CHECK(hipStreamSynchronize(s));
  host_step_ = step;
  mirrored_ = nullptr;     // a fresh x: its second block is rewritten by the next guided step
  return T2P_OK;
}

int Sampler::set_guidance(double w, int enabled) {
  T2P_REQUIRE(std::isfinite(w), "the guidance weight must be finite");
  T2P_REQUIRE(enabled == 0 || enabled == 1, "enabled is 0 or 1");
  if (enabled && w != 1.0 && !score2_) {
    score2_ = (float*)e_->pool().persistent((size_t)n_ * 2 * 4);
    if (!score2_) return T2P_ERR_HIP;
  }
  guidance_ = enabled != 0;
  w_ = w;
  mirrored_ = nullptr;
  if (graph_exec_) {       // the captured step holds the weight and the batch of its evaluation
    (void)hipGraphExecDestroy(graph_exec_);
    graph_exec_ = nullptr;
  }
  return T2P_OK;
}

int Sampler::set_context(const float* ctx, int B, int T, hipStream_t s) {
  T2P_REQUIRE(ctx && T > 0, "set_context arguments");
  T2P_REQUIRE(B == cfg_.batch, "the context batch must equal cfg.batch");
  have_context2_ = false;      // a failure below leaves the engine's text caches in an unknown state
  if (!guided()) return e_->set_context(ctx, B, T, s);
  T2P_TRY(ctx2_.project(e_, ctx, B, T, s));
  have_context2_ = true;
  return T2P_OK;
}

int Sampler::set_vp_tables(const float* label_f, const float* score_scale, const float* x_coef, const float* corr_alpha) {
  T2P_REQUIRE(cfg_.sde == T2P_SDE_VP, "VP tables belong to a sampler created with sde = T2P_SDE_VP");
  T2P_REQUIRE(label_f && score_scale && x_coef && corr_alpha, "null table");
  DevPool& pool = e_->pool();
  const size_t bytes = (size_t)cfg_.N * 4;
  float** dst[4] = {&vp_label_f_, &vp_score_scale_, &vp_x_coef_, &vp_alpha_};
  const float* src[4] = {label_f, score_scale, x_coef, corr_alpha};
  for (int i = 0; i < 4; ++i) {
    if (!*dst[i]) *dst[i] = (float*)pool.persistent(bytes);
    if (!*dst[i]) return T2P_ERR_HIP;
    T2P_HIP_CHECK(hipMemcpy(*dst[i], src[i], bytes, hipMemcpyHostToDevice));
  }
  return T2P_OK;
}

int Sampler::set_inpaint(const uint8_t* known, const float* data, const float* mean_coef_host, const float* std_host) {
  const bool ptrs = known && data, tabs = mean_coef_host && std_host;
  T2P_REQUIRE((known != nullptr) == (data != nullptr), "set_inpaint: known and data go together");
  T2P_REQUIRE((mean_coef_host != nullptr) == (std_host != nullptr), "set_inpaint: the mean_coef and std tables go together");
  T2P_REQUIRE(ptrs == tabs, "set_inpaint: the pointers and the tables go together (all null clears the replacement)");
  if (ptrs) {
    const size_t bytes = (size_t)cfg_.N * 4;
    if (!rp_mean_) {
      float* m = (float*)e_->pool().persistent(bytes);
      float* sd = (float*)e_->pool().persistent(bytes);
      if (!m || !sd) return T2P_ERR_HIP;
      rp_mean_ = m; rp_std_ = sd;
    }
    T2P_HIP_CHECK(hipMemcpy(rp_mean_, mean_coef_host, bytes, hipMemcpyHostToDevice));
    T2P_HIP_CHECK(hipMemcpy(rp_std_, std_host, bytes, hipMemcpyHostToDevice));
  }
  known_ = known; data_ = data;
  if (!ptrs) rp_noise_c_ = rp_noise_p_ = nullptr;
  return T2P_OK;
}

int Sampler::set_inpaint_noise(const float* after_corrector, const float* after_predictor) {
  T2P_REQUIRE(cfg_.n_steps_each == 1 || !after_corrector, "injected corrector-side noise supports n_steps_each == 1");
  T2P_REQUIRE(known_ || (!after_corrector && !after_predictor), "set_inpaint_noise: call t2p_sampler_set_inpaint first");
  rp_noise_c_ = after_corrector; rp_noise_p_ = after_predictor;
  return T2P_OK;
}

int Sampler::set_norm_allreduce(float* sums, t2p_allreduce_fn fn, void* user) {
  T2P_REQUIRE((sums == nullptr) == (fn == nullptr), "the sums buffer and the all-reduce callback go together");
  sums_ext_ = sums; allreduce_ = fn; allreduce_user_ = user;
  return T2P_OK;
}

// one iteration of the loop body of pc_sampler (sampling.py:279-285)
int Sampler::step(float* x, float* x_mean, const float* nc, const float* np, hipStream_t s) {
  T2P_REQUIRE(x, "x is null");
  T2P_REQUIRE(cfg_.n_steps_each == 1 || !nc, "injected corrector noise supports n_steps_each == 1");
  // the schedule tables hold N entries: a step past the end of the run is a caller error (t2p_sampler_reset rewinds)
  T2P_REQUIRE(host_step_ >= 0 && host_step_ < cfg_.N, "PC step index beyond sde.N: call t2p_sampler_reset before another run");
  // Langevin batch mean over global_batch chains (reference DataParallel run): needs the norm sums of the other
  // processes, i.e. the all-reduce hook; without it the mean runs over this process's chains
  T2P_REQUIRE(cfg_.global_batch == cfg_.batch || allreduce_, "global_batch > batch needs t2p_sampler_set_norm_allreduce");
  {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s) (void)hipStreamIsCapturing(s, &cap);
    if (cap == hipStreamCaptureStatusNone && eager_steps_ < (1 << 30)) ++eager_steps_;     // steps that really ran (step_graph / count_dispatches ask)
  }
  const int B = cfg_.batch;
  const bool vp = cfg_.sde == T2P_SDE_VP;
  T2P_REQUIRE(!vp || vp_label_f_, "VP SDE: call t2p_sampler_set_vp_tables first");
  float* sums = allreduce_ ? sums_ext_ : sums_;
  // Under guidance: one evaluation of [x ; x] at batch 2B per score, every update written to both blocks of x, the norms summed in
  // quads.  Nothing else differs: the guidance sum and the VP score scale are formed inside the norm and update kernels.
  const bool gd = guided();
  T2P_REQUIRE(!gd || have_context2_, "guided sampling: call t2p_sampler_set_context first (after t2p_sampler_set_guidance)");
  if (gd && mirrored_ != x) {     // first step on this buffer: the zero-context half of the evaluation reads a copy of x
    T2P_TRY(launch_ddim_mirror(x, x + n_, n_, s));
    mirrored_ = x;
  }
  float* out = gd ? score2_ : score_;
  float* x2 = gd ? x + n_ : nullptr;
  // score function (models/utils.py:138-171): VE = the network output at the integer label; VP = -output / std at the fractional one
  GuidedScore g;
  g.o_c = out; g.o_u = gd ? out + n_ : nullptr; g.w = (float)w_; g.w1 = (float)(1.0 - w_);
  g.scale_table = vp ? vp_score_scale_ : nullptr; g.step_counter = step_dev_; g.n_table = cfg_.N;
  auto score_fn = [&]() -> int {
    return e_->score(x, nullptr, step_dev_, out, gd ? 2 * B : B, s, nullptr, label_table_, vp ? vp_label_f_ : nullptr);
  };
  SdeUpdateArgs a;
  a.x = x; a.mask = mask_; a.x_initial = mask_ ? x_init_ : nullptr; a.x_out = x; a.n = n_;     // x_initial alone was always ignored
  // replacement inpainting: the known region is re-noised after the corrector (its last inner step) and after the predictor, inside
  // the update kernels; streams of the two draws: philox.h
  InpaintReplace rc;
  rc.known = known_; rc.data = data_; rc.mean_table = rp_mean_; rc.std_table = rp_std_; rc.step_counter = step_dev_; rc.n_table = cfg_.N;
  rc.seed = cfg_.seed;
  InpaintReplace rp = rc;
  rc.noise = rp_noise_c_; rc.stream = 0x80000000ull;
  rp.noise = rp_noise_p_; rp.stream = 0x80000001ull;
  for (int k = 0; k < cfg_.n_steps_each; ++k) {
    T2P_TRY(score_fn());
    a.noise = nc;
    if (!nc) {
      T2P_TRY(launch_philox_normal(noise_, n_, cfg_.seed, 2ull * k + 2, step_dev_, s));
      a.noise = noise_;
    }
    T2P_TRY(launch_langevin_norms(g, a.noise, B, per_sample_, sq_ws_, sums, gd ? 4 : 1, s));
    if (allreduce_) {     // sum_b ||grad_b||, sum_b ||noise_b|| over every process's chains (SURVEY 8(e) option B)
      const int rc = allreduce_(sums, (void*)s, allreduce_user_);
      if (rc != 0) { set_last_error("the norm all-reduce callback failed with status " + std::to_string(rc)); return T2P_ERR_STATE; }
    }
    T2P_TRY(launch_langevin_update(a, g, x2, sums, (float)(allreduce_ ? cfg_.global_batch : B), (float)cfg_.snr, 1.f, s,
                                   vp ? vp_alpha_ : nullptr, known_ && k == cfg_.n_steps_each - 1 ? &rc : nullptr));
  }
  T2P_TRY(score_fn());
  a.noise = np;
  if (!np) {
    T2P_TRY(launch_philox_normal(noise_, n_, cfg_.seed, 1, step_dev_, s));
    a.noise = noise_;
  }
  a.x_mean_out = x_mean ? x_mean : xmean_;
  T2P_TRY(launch_predictor_update(a, g, x2, g_table_, 0.f, cfg_.probability_flow, s, vp ? vp_x_coef_ : nullptr, 1.f, known_ ? &rp : nullptr));
  T2P_TRY(launch_add_int(step_dev_, 1, s));
  ++host_step_;
  return T2P_OK;
}

Sampler::~Sampler() {
  if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
}

int Sampler::step_graph(float* x, float* x_mean, hipStream_t s) {
  T2P_REQUIRE(x && x_mean, "step_graph needs explicit x and x_mean buffers");
  T2P_REQUIRE(!allreduce_, "the captured step does not run the norm all-reduce hook: use t2p_sampler_step");
  T2P_REQUIRE(host_step_ >= 0 && host_step_ < cfg_.N, "PC step index beyond sde.N: call t2p_sampler_reset before another run");
  T2P_REQUIRE(!rp_noise_c_ && !rp_noise_p_, "the captured step draws on the device: clear t2p_sampler_set_inpaint_noise");
  // one eager step first: fills the activation pool (no hipMalloc under capture); step() counts it.  Guided: also the first step
  // after a reset, which writes the second block of x once (the captured step does not)
  if (eager_steps_ < 1 || (guided() && mirrored_ != x))
    return step(x, x_mean, nullptr, nullptr, s);
  if (graph_exec_ && (graph_x_ != x || graph_xm_ != x_mean || graph_mask_ != mask_ || graph_seed_ != cfg_.seed || graph_known_ != known_ ||
                      graph_data_ != data_)) {
    (void)hipGraphExecDestroy(graph_exec_);
    graph_exec_ = nullptr;
  }
  if (!graph_exec_) {
    hipGraph_t graph = nullptr;
    T2P_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int step_before = host_step_;
    const int rc = step(x, x_mean, nullptr, nullptr, s);
    host_step_ = step_before;            // the capture enqueued nothing: the replay below is the step
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc != T2P_OK) {                  // a partial capture is dropped, the mirror of the device counter is untouched
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    T2P_HIP_CHECK(ec);
    T2P_HIP_CHECK(hipGraphInstantiate(&graph_exec_, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    graph_x_ = x; graph_xm_ = x_mean; graph_mask_ = mask_; graph_seed_ = cfg_.seed; graph_known_ = known_; graph_data_ = data_;
  }
  T2P_HIP_CHECK(hipGraphLaunch(graph_exec_, s));
  ++host_step_;
  return T2P_OK;
}

// number of kernel / memory nodes one PC step enqueues: the step is captured into a hipGraph (nothing executes) and its nodes
// are counted.  Needs a non-default stream and a filled activation pool (one eager step before).
int Sampler::count_dispatches(float* x, float* x_mean, hipStream_t s, int* n_out) {
  T2P_REQUIRE(x && x_mean && n_out, "null argument");
  T2P_REQUIRE(eager_steps_ >= 1, "count_dispatches captures a step: run one eager step first (it sizes the pool and builds per-block weight copies)");
  T2P_REQUIRE(!allreduce_, "the captured step does not run the norm all-reduce hook");
  T2P_REQUIRE(host_step_ >= 0 && host_step_ < cfg_.N, "PC step index beyond sde.N: call t2p_sampler_reset before another run");
  hipGraph_t graph = nullptr;
  T2P_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int step_before = host_step_;
  const float* mirrored_before = mirrored_;
  const int rc = step(x, x_mean, nullptr, nullptr, s);
  host_step_ = step_before;
  mirrored_ = mirrored_before;         // a mirror launch of the first guided step was counted, not run
  const hipError_t ec = hipStreamEndCapture(s, &graph);
  if (rc != T2P_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  T2P_HIP_CHECK(ec);
  size_t n = 0;
  const hipError_t eg = hipGraphGetNodes(graph, nullptr, &n);
  (void)hipGraphDestroy(graph);
  T2P_HIP_CHECK(eg);
  *n_out = (int)n;
  return T2P_OK;
}

int Sampler::run(float* x, float* out, int prior_given, int n_steps, hipStream_t s) {
  T2P_REQUIRE(x && out, "null pointer");
  if (n_steps <= 0 || n_steps > cfg_.N) n_steps = cfg_.N;
  T2P_TRY(reset(0, s));
  if (!prior_given) {
    // VESDE.prior_sampling (sde_lib.py:229-230) then where(mask, x, x_initial)
    T2P_TRY(launch_philox_normal(x, n_, cfg_.seed, 0, nullptr, s));
    if (cfg_.sde == T2P_SDE_VE) T2P_TRY(launch_scale(x, n_, (float)cfg_.sigma_max, s));     // VP prior: N(0, 1) (sde_lib.py:133-134)
    if (known_) T2P_TRY(launch_put_known(x, known_, data_, n_, s));     // x = known ? d : prior (inpainting.py:66), then the condition
    if (mask_) T2P_TRY(launch_apply_mask(x, mask_, x_init_, n_, s));
  }
  for (int i = 0; i < n_steps; ++i) T2P_TRY(step(x, xmean_, nullptr, nullptr, s));
  const float* src = cfg_.denoise ? xmean_ : x;
  T2P_HIP_CHECK(hipMemcpyAsync(out, src, (size_t)n_ * 4, hipMemcpyDeviceToDevice, s));
  if (cfg_.denoise && mask_) T2P_TRY(launch_apply_mask(out, mask_, x_init_, n_, s));   // sampling.py:287
  return T2P_OK;
}

}  // namespace t2p
