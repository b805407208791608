// DDIM sampling with classifier-free guidance on the score engine: the strided loop of the reference's second sampler
// (sampler/diffusion_sampler.py:72-142; twin model/diffusion_sampler.py).  One elementwise kernel per step does the guidance
// sum, the clean-sample prediction, its static clipping, the DDIM move, the conditional re-masking and the noise draw; the
// host loop (class Ddim) evaluates the network ONCE per step on [x ; x] under the context [ctx ; 0] at batch 2B.
#include "ddim.h"
#include "update_loop.h"

#include <cmath>

namespace t2p {

// one element, rounded where the reference's float32 tensor expressions round (diffusion_sampler.py:141-142, 133, 110-112); eps is
// the guidance sum w eps_c + w1 eps_u of update_loop.h's guided_score at scale 1 (diffusion_sampler.py:128)
__device__ inline float ddim_element(const DdimUpdateArgs& a, float x, float eps, float z, float* x0_out) {
#pragma clang fp contract(off)
  const float px = a.sqrt_recip * x, pe = a.sqrt_recipm1 * eps;
  float x0 = px - pe;
  if (a.clip) x0 = x0 < -1.f ? -1.f : (x0 > 1.f ? 1.f : x0);     // torch.clamp: a NaN stays a NaN
  *x0_out = x0;
  if (a.last) return x0;
  const float t0 = x0 * a.sqrt_an, t1 = a.c * eps, t2 = a.sigma * z;
  const float s01 = t0 + t1;
  return s01 + t2;
}

// The quad loop of update_loop.h with ddim_element as its update and x0 as its second output.  z: the given draws; nothing on the
// last step; else drawn in the loop, unless sigma == 0 (the term is sigma * 0, nothing is drawn).
template <bool VEC>
__global__ __launch_bounds__(256) void ddim_update_kernel(DdimUpdateArgs a) {
  SdeUpdateArgs u;
  u.x = a.x; u.noise = a.last ? nullptr : a.z; u.mask = a.mask; u.x_initial = a.x_initial; u.x_out = a.x_out; u.x_mean_out = a.x0_out;
  u.n = a.n;
  GuidedScore g;
  g.o_c = a.eps_c; g.o_u = a.eps_u; g.w = a.w; g.w1 = a.w1;
  QuadDraw d;
  d.on = !a.last && !a.z && a.sigma != 0.f; d.seed = a.seed; d.stream_id = a.stream_id;
  update_loop<VEC, true>(u, g, a.x_out2, d, [=](float x, float eps, float z, float* x0) { return ddim_element(a, x, eps, z, x0); });
}

int launch_ddim_update(const DdimUpdateArgs& a, hipStream_t s) {
  T2P_REQUIRE(a.x && a.eps_c && a.x_out && a.n > 0, "ddim_update arguments");
  T2P_REQUIRE((a.mask == nullptr) == (a.x_initial == nullptr), "mask and x_initial go together");
  T2P_REQUIRE(a.clip == 0 || a.clip == 1, "clip is 0 or 1");
  T2P_REQUIRE(a.last == 0 || a.last == 1, "last is 0 or 1");
  const dim3 grid(ew_grid((a.n + 3) / 4));
  if (quad_vec_ok(a.n, {a.x, a.eps_c, a.eps_u, a.z, a.x_initial, a.x_out, a.x_out2, a.x0_out}, a.mask))
    hipLaunchKernelGGL(ddim_update_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(ddim_update_kernel<false>, grid, dim3(256), 0, s, a);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void ddim_mirror_kernel(const float* src, float* dst, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = src[i];
}
int launch_ddim_mirror(const float* src, float* dst, long n, hipStream_t s) {
  T2P_REQUIRE(src && dst && n > 0, "ddim_mirror arguments");
  hipLaunchKernelGGL(ddim_mirror_kernel, dim3(ew_grid(n)), dim3(256), 0, s, src, dst, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void ddim_context2_kernel(const float* ctx, float* out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    out[i] = ctx[i];
    out[n + i] = 0.f;
  }
}
int launch_ddim_context2(const float* ctx, float* out, long n, hipStream_t s) {
  T2P_REQUIRE(ctx && out && n > 0, "ddim_context2 arguments");
  hipLaunchKernelGGL(ddim_context2_kernel, dim3(ew_grid(n)), dim3(256), 0, s, ctx, out, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ------------------------------------------------------------------------------------------------
// the loop of DiffusionSampler.ddim_sample (diffusion_sampler.py:87-114) over the step table the Python mirror computed
Ddim::~Ddim() {
  (void)hipFree(labels_);
  (void)hipFree(eps_);
}

GuidedContext::~GuidedContext() { (void)hipFree(ctx2_); }

int GuidedContext::project(Engine* e, const float* ctx, int B, int T, hipStream_t s) {
  const size_t half = (size_t)B * T * e->cfg().context_dim;
  if (2 * half > floats_) {
    float* p = nullptr;
    T2P_HIP_CHECK(hipMalloc((void**)&p, 2 * half * 4));
    (void)hipFree(ctx2_);     // (waits for the work that may still read it)
    ctx2_ = p;
    floats_ = 2 * half;
  }
  T2P_TRY(launch_ddim_context2(ctx, ctx2_, (long)half, s));
  return e->set_context(ctx2_, 2 * B, T, s);
}

int Ddim::init(const t2p_ddim_step_row* table) {
  T2P_REQUIRE(e_->finalized(), "finalize the engine first");
  T2P_REQUIRE(table, "null step table");
  T2P_REQUIRE(cfg_.sampling_steps >= 1, "sampling_steps must be at least 1");
  T2P_REQUIRE(cfg_.eta >= 0.0 && cfg_.eta <= 1.0, "eta must lie in [0, 1]");       // also refuses a NaN
  T2P_REQUIRE(std::isfinite(cfg_.w), "the guidance weight must be finite");
  T2P_REQUIRE(cfg_.timesteps >= 1 && cfg_.timesteps <= e_->cfg().num_scales, "timesteps must lie in [1, model.num_scales]");
  T2P_REQUIRE(cfg_.batch > 0 && cfg_.batch <= (1 << 20), "batch");
  T2P_REQUIRE(cfg_.clip == 0 || cfg_.clip == 1, "clip is 0 or 1");
  const int S = cfg_.sampling_steps, B2 = 2 * cfg_.batch;
  for (int i = 0; i < S; ++i) {
    T2P_REQUIRE(table[i].t >= 0 && table[i].t < e_->cfg().num_scales, "time label outside [0, num_scales)");
    T2P_REQUIRE(table[i].last == 0 || table[i].last == 1, "last is 0 or 1");
  }
  table_.assign(table, table + S);
  const t2p_model_config& m = e_->cfg();
  n_ = (long)m.num_channels * m.max_res_num * m.max_res_num * cfg_.batch;
  std::vector<int32_t> lab((size_t)S * B2);
  for (int i = 0; i < S; ++i) std::fill(lab.begin() + (size_t)i * B2, lab.begin() + (size_t)(i + 1) * B2, table_[i].t);
  T2P_HIP_CHECK(hipMalloc((void**)&labels_, lab.size() * 4));
  T2P_HIP_CHECK(hipMalloc((void**)&eps_, (size_t)n_ * 2 * 4));
  T2P_HIP_CHECK(hipMemcpy(labels_, lab.data(), lab.size() * 4, hipMemcpyHostToDevice));
  return T2P_OK;
}

int Ddim::set_context(const float* ctx, int B, int T, hipStream_t s) {
  T2P_REQUIRE(ctx && T > 0, "set_context arguments");
  T2P_REQUIRE(B == cfg_.batch, "the context batch must equal cfg.batch");
  if (!guided()) {          // w == 1: 1 eps_c + 0 eps_u == eps_c, the zero-context half is never evaluated
    T2P_TRY(e_->set_context(ctx, B, T, s));
    have_context_ = true;
    return T2P_OK;
  }
  have_context_ = false;      // a failure below leaves the engine's text caches in an unknown state
  T2P_TRY(ctx2_.project(e_, ctx, B, T, s));
  have_context_ = true;
  return T2P_OK;
}

int Ddim::reset(int step) {
  T2P_REQUIRE(step >= 0 && step < cfg_.sampling_steps, "step out of range");
  host_step_ = step;
  mirrored_ = nullptr;
  return T2P_OK;
}

int Ddim::step(float* x, float* x0_out, const float* noise, hipStream_t s) {
  T2P_REQUIRE(x, "x is null");
  T2P_REQUIRE(have_context_, "call t2p_ddim_set_context first");
  T2P_REQUIRE(host_step_ >= 0 && host_step_ < cfg_.sampling_steps, "DDIM step index beyond the step table: call t2p_ddim_reset before another run");
  const t2p_ddim_step_row& r = table_[host_step_];
  const int B = cfg_.batch;
  const bool g = guided();
  if (g && mirrored_ != x) {     // first step on this buffer: the zero-context half of the evaluation reads a copy of x
    T2P_TRY(launch_ddim_mirror(x, x + n_, n_, s));
    mirrored_ = x;
  }
  T2P_TRY(e_->score(x, labels_ + (size_t)host_step_ * 2 * B, nullptr, eps_, g ? 2 * B : B, s));
  DdimUpdateArgs a;
  a.x = x; a.eps_c = eps_; a.eps_u = g ? eps_ + n_ : nullptr; a.z = noise; a.mask = mask_; a.x_initial = x_init_;
  a.x_out = x; a.x_out2 = g ? x + n_ : nullptr; a.x0_out = x0_out; a.n = n_;
  a.w = (float)cfg_.w; a.w1 = (float)(1.0 - cfg_.w);
  a.sqrt_recip = r.sqrt_recip; a.sqrt_recipm1 = r.sqrt_recipm1; a.sqrt_an = r.sqrt_an; a.c = r.c; a.sigma = r.sigma;
  a.clip = cfg_.clip; a.last = r.last;
  a.seed = cfg_.seed; a.stream_id = (unsigned long long)host_step_ + 1;     // draw 0 is the prior
  T2P_TRY(launch_ddim_update(a, s));
  ++host_step_;
  return T2P_OK;
}

int Ddim::run(float* x, float* out, int prior_given, int n_steps, hipStream_t s) {
  T2P_REQUIRE(x && out, "null pointer");
  T2P_REQUIRE(have_context_, "call t2p_ddim_set_context first");
  if (n_steps <= 0 || n_steps > cfg_.sampling_steps) n_steps = cfg_.sampling_steps;
  T2P_TRY(reset(0));
  if (!prior_given) {            // torch.randn(shape) (diffusion_sampler.py:91), then the condition
    T2P_TRY(launch_philox_normal(x, n_, cfg_.seed, 0, nullptr, s));
    if (mask_) T2P_TRY(launch_apply_mask(x, mask_, x_init_, n_, s));
  }
  for (int i = 0; i < n_steps; ++i) T2P_TRY(step(x, nullptr, nullptr, s));
  if (out != x) T2P_TRY(launch_ddim_mirror(x, out, n_, s));
  return T2P_OK;
}

}  // namespace t2p
