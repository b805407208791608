// Predictor-corrector sampling (score_sde_pytorch/sampling.py:213-291): the fused host-side loop over a finalized Engine; its noise streams: philox.h.
#pragma once
#include "ddim.h"
#include "engine.h"

namespace t2p {

class Sampler {
 public:
  Sampler(Engine* e, const t2p_sampler_config& cfg);
  int init(const float* g_table_host, const int32_t* label_table_host);
  int set_condition(const uint8_t* mask, const float* x_initial) { mask_ = mask; x_init_ = x_initial; return T2P_OK; }
  void set_seed(uint64_t seed) { cfg_.seed = seed; }
  // global-batch Langevin step size (reference under DataParallel, sampling.py:193-195): `sums` is a caller-owned
  // device float[2] the norm sums of this process's chains are written to; `fn` must sum it over all processes
  // in stream order before returning control (e.g. one RCCL all_reduce enqueued on `stream`)
  int set_norm_allreduce(float* sums, t2p_allreduce_fn fn, void* user);
  // VP SDE (sde_lib.py:106-157) in the fused loop: per-step host tables of N floats (see t2p_sampler_set_vp_tables)
  int set_vp_tables(const float* label_f, const float* score_scale, const float* x_coef, const float* corr_alpha);
  // classifier-free guidance (reference sampler/diffusion_sampler.py:128): every score of the loop becomes w out(ctx) + (1 - w) out(0),
  // from ONE evaluation of [x ; x] under [ctx ; 0] at batch 2B.  x then has room for 2B samples (see t2p_sampler_step).
  int set_guidance(double w, int enabled);
  int set_context(const float* ctx, int B, int T, hipStream_t s);
  // replacement inpainting (score_sde_pytorch/inpainting.py): after every corrector and predictor update the known region becomes
  // mean_coef[i] data + std[i] z at loop step i; host tables of N floats.  All null clears it.  The pointers are borrowed.
  int set_inpaint(const uint8_t* known, const float* data, const float* mean_coef_host, const float* std_host);
  // the z of the two replacements of the next steps (fixture replay); null = drawn on the device (philox.h)
  int set_inpaint_noise(const float* after_corrector, const float* after_predictor);
  bool guided() const { return guidance_ && w_ != 1.0; }     // w == 1: 1 a + 0 b == a, the plain path at batch B
  int reset(int step, hipStream_t s);
  int step(float* x, float* x_mean, const float* nc, const float* np, hipStream_t s);
  // step() through a captured hipGraph (device noise only): first call with a given (x, x_mean,
  // condition) captures, later calls replay.  The step reads its index from the device counter.
  int step_graph(float* x, float* x_mean, hipStream_t s);
  int run(float* x, float* out, int prior_given, int n_steps, hipStream_t s);
  int count_dispatches(float* x, float* x_mean, hipStream_t s, int* n_out);
  ~Sampler();

 private:
  Engine* e_;
  t2p_sampler_config cfg_;
  const uint8_t* mask_ = nullptr;
  const float* x_init_ = nullptr;
  int* step_dev_ = nullptr;
  float* g_table_ = nullptr;
  float* score_ = nullptr;
  float* noise_ = nullptr;
  float* sq_ws_ = nullptr;
  float* sums_ = nullptr;
  float* xmean_ = nullptr;
  int* label_table_ = nullptr;     // device int[N]: time label of loop step i
  float* vp_label_f_ = nullptr;    // VP: device float[N] each
  float* vp_score_scale_ = nullptr;
  float* vp_x_coef_ = nullptr;
  float* vp_alpha_ = nullptr;
  int host_step_ = 0;              // host mirror of *step_dev_ (bounds check: the tables have N entries)
  float* sums_ext_ = nullptr;
  t2p_allreduce_fn allreduce_ = nullptr;
  void* allreduce_user_ = nullptr;
  uint64_t graph_seed_ = 0;
  long n_ = 0, per_sample_ = 0;
  hipGraphExec_t graph_exec_ = nullptr;
  float* graph_x_ = nullptr;
  float* graph_xm_ = nullptr;
  const uint8_t* graph_mask_ = nullptr;
  const uint8_t* graph_known_ = nullptr;
  const float* graph_data_ = nullptr;
  const uint8_t* known_ = nullptr;    // replacement inpainting: 1 = known, with data_
  const float* data_ = nullptr;
  float* rp_mean_ = nullptr;          // device float[N] each: a_i and s_i of marginal_prob at loop step i
  float* rp_std_ = nullptr;
  const float* rp_noise_c_ = nullptr; // injected z of the replacement after the corrector / the predictor
  const float* rp_noise_p_ = nullptr;
  int eager_steps_ = 0;
  bool guidance_ = false;
  double w_ = 1.0;
  float* score2_ = nullptr;           // device float[2 n]: the network output at batch 2B, text half then zero-context half
  GuidedContext ctx2_;                // [ctx ; 0]
  bool have_context2_ = false;        // the engine holds the projections of ctx2_
  const float* mirrored_ = nullptr;   // the x whose second block holds a copy of the first (null after reset)
};

}  // namespace t2p

struct t2p_sampler { t2p::Sampler impl; t2p_sampler(t2p::Engine* e, const t2p_sampler_config& c) : impl(e, c) {} };
