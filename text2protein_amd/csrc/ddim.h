// Strided DDIM sampling with classifier-free guidance (reference sampler/diffusion_sampler.py:72-142): the elementwise update
// kernel's launcher and the host-side loop over a finalized Engine.
#pragma once
#include <vector>

#include "engine.h"

namespace t2p {

// One DDIM update over n elements (diffusion_sampler.py:96-112, 128-142), every per-step scalar by value:
//   eps = w eps_c + w1 eps_u (eps_u null: eps = eps_c);  x0 = sqrt_recip x - sqrt_recipm1 eps, clamped to [-1, 1] when clip;
//   x_next = x0 (last) or x0 sqrt_an + c eps + sigma z;  x_next = mask ? x_next : x_initial.
// Products and sums are rounded where the reference's float32 tensors round them (no contraction into FMAs).
struct DdimUpdateArgs {
  const float* x = nullptr;
  const float* eps_c = nullptr;          // network output under the text context
  const float* eps_u = nullptr;          // under the zero context; null = no guidance sum
  const float* z = nullptr;              // standard normal draws; null = drawn in the kernel (seed, stream_id); unused when last
  const unsigned char* mask = nullptr;   // conditional_mask (1 = free), may be null
  const float* x_initial = nullptr;
  float* x_out = nullptr;                // may alias x
  float* x_out2 = nullptr;               // optional second copy of x_next (the other half of a 2B batch)
  float* x0_out = nullptr;               // optional: the (clamped) predicted clean sample
  long n = 0;
  float w = 1.f, w1 = 0.f;               // guidance weight and (1 - w) as the reference rounds it (from the double)
  float sqrt_recip = 1.f, sqrt_recipm1 = 0.f, sqrt_an = 1.f, c = 0.f, sigma = 0.f;
  int clip = 1, last = 0;
  unsigned long long seed = 0, stream_id = 0;
};
int launch_ddim_update(const DdimUpdateArgs& a, hipStream_t s);
// dst[i] = src[i] (the second half of the [x ; x] input of a guided evaluation; the result copy of a run)
int launch_ddim_mirror(const float* src, float* dst, long n, hipStream_t s);
// out[i] = ctx[i], out[n + i] = 0: the context of a guided evaluation, [ctx ; cond * 0] (diffusion_sampler.py:128)
int launch_ddim_context2(const float* ctx, float* out, long n, hipStream_t s);

// The context of a guided evaluation, owned by a sampler: [ctx ; 0] built on the device and projected through the engine at batch 2B
// (to_k / to_v have no bias, so the zero half gives zero keys and values, as `cond * 0` does).  One builder for the DDIM loop and
// the guided predictor-corrector loop.
class GuidedContext {
 public:
  ~GuidedContext();
  // ctx: device fp32 [B][T][context_dim].  On failure the engine's text caches are in an unknown state: set again before a step.
  int project(Engine* e, const float* ctx, int B, int T, hipStream_t s);

 private:
  float* ctx2_ = nullptr;       // device float[2 B T D]
  size_t floats_ = 0;
};

class Ddim {
 public:
  Ddim(Engine* e, const t2p_ddim_config& cfg) : e_(e), cfg_(cfg) {}
  ~Ddim();
  int init(const t2p_ddim_step_row* table);
  void set_seed(uint64_t seed) { cfg_.seed = seed; }
  int set_condition(const uint8_t* mask, const float* x_initial) { mask_ = mask; x_init_ = x_initial; return T2P_OK; }
  int set_context(const float* ctx, int B, int T, hipStream_t s);
  int reset(int step);
  int step(float* x, float* x0_out, const float* noise, hipStream_t s);
  int run(float* x, float* out, int prior_given, int n_steps, hipStream_t s);
  bool guided() const { return cfg_.w != 1.0; }

 private:
  Engine* e_;
  t2p_ddim_config cfg_;
  std::vector<t2p_ddim_step_row> table_;
  const uint8_t* mask_ = nullptr;
  const float* x_init_ = nullptr;
  int* labels_ = nullptr;       // device int[sampling_steps][2 batch]: the time label of loop step i for every row of the evaluation
  float* eps_ = nullptr;        // device float[2 n]: the network output, text half then zero-context half
  GuidedContext ctx2_;          // [ctx ; 0]
  bool have_context_ = false;
  const float* mirrored_ = nullptr;   // the x whose second half holds a copy of the first (null after reset)
  int host_step_ = 0;
  long n_ = 0;
};

}  // namespace t2p

struct t2p_ddim { t2p::Ddim impl; t2p_ddim(t2p::Engine* e, const t2p_ddim_config& c) : impl(e, c) {} };
