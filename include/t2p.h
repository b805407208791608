/* t2p.h -- C ABI of libt2p_hip.so: the text2protein reverse-diffusion sampling path on MI355X.
 *
 * The reference (szhan227/text2protein) has no FFI layer; its seam for this path is a set of
 * Python callables.  Each entry point below names the reference
 * interface it stands in for.  All pointers marked "device" are HIP device pointers owned by
 * the caller; nothing is retained beyond the call unless stated.  `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  Every function returns 0 on success or a
 * non-zero status; t2p_last_error() then returns a message for the calling thread.
 * There is no CPU fallback: every compute entry point launches HIP kernels.
 */
#ifndef T2P_H_
#define T2P_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2P_DTYPE_F32 0   /* exact-f32 MFMA (v_mfma_f32_32x32x2_f32)      */
#define T2P_DTYPE_BF16 1  /* bf16 operands, fp32 accumulate                */
#define T2P_DTYPE_F16 2   /* fp16 operands, fp32 accumulate                */

#define T2P_SDE_VE 0
#define T2P_SDE_VP 1
#define T2P_SDE_SUBVP 2   /* training step only (t2p_train_set_sde) */

/* Flat view of the YAML keys the score network reads
 * (reference score_sde_pytorch/models/ncsnpp.py:74-217, configs/test_config.yml). */
typedef struct t2p_model_config {
  int32_t num_channels;        /* data.num_channels                        */
  int32_t max_res_num;         /* data.max_res_num (map side L)            */
  int32_t nf;                  /* model.nf                                 */
  int32_t num_res_blocks;      /* model.num_res_blocks                     */
  int32_t n_ch_mult;           /* len(model.ch_mult), <= 8                 */
  int32_t ch_mult[8];
  int32_t n_attn_resolutions;  /* len(model.attn_resolutions), <= 8        */
  int32_t attn_resolutions[8];
  int32_t n_heads;             /* model.n_heads                            */
  int32_t context_dim;         /* model.context_dim                        */
  int32_t num_scales;          /* model.num_scales (N)                     */
  double sigma_min, sigma_max; /* model.sigma_{min,max}                    */
  int32_t skip_rescale;        /* model.skip_rescale                       */
  int32_t scale_by_sigma;      /* model.scale_by_sigma                     */
  int32_t compute_dtype;       /* T2P_DTYPE_*                              */
} t2p_model_config;

typedef struct t2p_engine t2p_engine;    /* the score network: UNetModel (ncsnpp.py:71-263) */
typedef struct t2p_sampler t2p_sampler;  /* the PC loop: get_pc_sampler (sampling.py:213-291) */

const char* t2p_last_error(void);
/* number of visible HIP devices, or -1 (no driver / no GPU).  Does not create a context. */
int t2p_device_count(void);

/* ---- score network ------------------------------------------------------------------------
 * t2p_engine_create      <- UNetModel.__init__ / get_model   (ncsnpp.py:74-217, score_sde_pytorch/utils.py:4-9)
 * t2p_engine_load_param  <- load_state_dict of one tensor    (score_sde_pytorch/utils.py:14);
 *                           `name` is the reference state-dict key, with or without "module."
 * t2p_engine_finalize    <- end of restore_checkpoint: fails if any tensor is missing
 * t2p_engine_set_context <- the `context=` argument          (sampling_6d.py:137,152): projects
 *                           the frozen text embedding through every to_k / to_v once
 * t2p_engine_score       <- model(x, labels, context)        (ncsnpp.py:220-263)                  */
int t2p_engine_create(const t2p_model_config* cfg, t2p_engine** out);
void t2p_engine_destroy(t2p_engine* e);
int t2p_engine_num_params(const t2p_engine* e);
/* name and shape (ndim <= 4) of expected tensor i, in reference parameters() order */
int t2p_engine_param_info(const t2p_engine* e, int i, const char** name, int64_t shape[4], int* ndim);
int t2p_engine_load_param(t2p_engine* e, const char* name, const float* host_data, const int64_t* shape, int ndim);
int t2p_engine_finalize(t2p_engine* e);
/* The weights from a flat fp32 DEVICE buffer in parameters() order (n = the table's total element count, else refused with nothing
 * changed), packed into the engine's layouts by kernels on `stream`: bit for bit what t2p_engine_load_param of the same numbers +
 * t2p_engine_finalize leave.  Any number of times, on an engine loaded either way: a later call overwrites the same buffers in place
 * (no allocation, no pointer changes: captured step graphs stay valid, t2p_engine_device_bytes is unchanged) and drops the cached text
 * projections, so t2p_engine_score is refused until t2p_engine_set_context ran again.  Does not wait for the stream. */
int t2p_engine_load_flat(t2p_engine* e, const float* device_flat, int64_t n, void* stream);
/* The last weight load, host or device: bytes its packings read, bytes they wrote, and how many packings it ran (for a device load:
 * the launches it enqueued).  tools/bench_refresh.py sets the refresh time against these. */
int t2p_engine_load_stats(const t2p_engine* e, int64_t out3[3]);
/* context: device fp32 [batch][tokens][context_dim] */
int t2p_engine_set_context(t2p_engine* e, const float* context, int batch, int tokens, void* stream);
/* x: device fp32 (batch, C, L, L); labels: device int32 [batch] time labels (index into the
 * descending sigma table); out: device fp32 (batch, C, L, L) = network output / sigma[label].
 * Range precondition of the 16-bit engines: with sigma_max <= 4096 the input convolution runs on f16 operand pairs and needs
 * |x| <= 65504 (a VE state stays within a few sigma_max); larger magnitudes saturate to that bound -- finite but wrong -- rather
 * than producing inf / NaN.  The f32 engine has no such bound. */
int t2p_engine_score(t2p_engine* e, const float* x, const int32_t* labels, float* out, int batch, void* stream);
/* as t2p_engine_score, with optional fractional time values for the sinusoidal embedding: the VP
 * branch of get_score_fn passes labels = t * (N - 1) as floats (models/utils.py:150-152); the
 * model embeds the float and indexes its sigma table with the truncated value (ncsnpp.py:223-224).
 * labels_f: device fp32 [batch] or NULL (= embed the integer labels). */
int t2p_engine_score_ex(t2p_engine* e, const float* x, const int32_t* labels, const float* labels_f, float* out,
                        int batch, void* stream);
/* bytes of device memory currently held (weights + cached activations) */
int64_t t2p_engine_device_bytes(const t2p_engine* e);
/* activation buffers the LAST score evaluation / set_context left checked out and the engine took back at its end: 0 after every
 * complete evaluation (a leak check for tests); > 0 only after a call that failed half-way */
int t2p_engine_pool_reclaimed(const t2p_engine* e);

/* ---- predictor-corrector sampler ------------------------------------------------------------
 * t2p_sampler_create        <- get_sampling_fn / get_pc_sampler (sampling.py:78-104, 213-243)
 * t2p_sampler_set_condition <- what sampling.py:259-277 reduces `condition` to:
 *                              conditional_mask (1 = evolves) and x_initial
 * t2p_sampler_step          <- one iteration of the loop body  (sampling.py:279-285)
 * t2p_sampler_run           <- pc_sampler(model, condition, context) (sampling.py:245-289)         */
typedef struct t2p_sampler_config {
  int32_t sde;               /* T2P_SDE_VE (every shipped config) or T2P_SDE_VP                  */
  int32_t N;                 /* sde.N = model.num_scales                                          */
  double sigma_min, sigma_max, beta_min, beta_max;
  double snr;                /* sampling.snr                                                      */
  int32_t n_steps_each;      /* sampling.n_steps_each                                             */
  int32_t probability_flow;  /* sampling.probability_flow                                         */
  int32_t denoise;           /* sampling.noise_removal                                            */
  double eps;                /* integrate to eps (1e-5 for VE, sampling_6d.py:79)                 */
  int32_t batch;             /* chains held by this process                                       */
  int32_t global_batch;      /* chains the Langevin batch-mean runs over (>= batch; > batch needs
                                t2p_sampler_set_norm_allreduce)                                   */
  uint64_t seed;             /* on-device Philox noise                                            */
} t2p_sampler_config;

/* g_table: optional host float[N], G_i of step i as the reference computes it in float32
 * (sde_lib.py:237-245); NULL = computed here in double.
 * label_table: optional host int32[N], the time label the score network receives at loop step i,
 * round((T - linspace(T, eps, N)[i]) (N - 1)) in the reference's float32 arithmetic (sampling.py:257,
 * models/utils.py:159-171); NULL = computed here in double from cfg->eps.  (It equals i only for tiny eps.) */
int t2p_sampler_create(t2p_engine* e, const t2p_sampler_config* cfg, const float* g_table, const int32_t* label_table,
                       t2p_sampler** out);
void t2p_sampler_destroy(t2p_sampler* s);
/* Seed of the on-device Philox noise of the following steps.  The reference draws fresh torch.randn noise on
 * every call of pc_sampler; the Python mirror derives one seed per (seed, call index) and sets it here. */
int t2p_sampler_set_seed(t2p_sampler* s, uint64_t seed);
/* VP SDE (VPSDE, sde_lib.py:106-157; score function models/utils.py:138-157; Langevin alpha sampling.py:184-186) in the fused
 * loop.  A sampler created with cfg.sde = T2P_SDE_VP takes g_table[i] = sqrt(beta_k) and label_table[i] = floor(t_i (N - 1)) at
 * t2p_sampler_create and, here, four more host tables of N floats for loop step i (t_i = linspace(T, eps, N)[i], k = the
 * reference's truncated timestep): label_f = t_i (N - 1) (the fractional label the network embeds), score_scale = -1 /
 * sqrt_1m_alphas_cumprod[label] (score = -model / std), x_coef = 2 - sqrt(alpha_k) (x - f with f = (sqrt(alpha) - 1) x),
 * corr_alpha = alpha_k. */
int t2p_sampler_set_vp_tables(t2p_sampler* s, const float* label_f, const float* score_scale, const float* x_coef, const float* corr_alpha);
/* Global-batch Langevin step size (the reference's DataParallel run takes the norm means over the whole batch,
 * sampling.py:193-195; cfg.global_batch > cfg.batch): every corrector step writes {sum_b ||grad_b||,
 * sum_b ||noise_b||} of this process's chains to `device_sums2` (caller-owned device float[2]) and calls
 * fn(device_sums2, stream, user), which must sum the two floats over all processes in stream order (one RCCL
 * all_reduce) and return 0.  NULL, NULL, NULL removes the hook. */
typedef int (*t2p_allreduce_fn)(float* device_sums2, void* stream, void* user);
int t2p_sampler_set_norm_allreduce(t2p_sampler* s, float* device_sums2, t2p_allreduce_fn fn, void* user);
/* mask: device uint8 (B,C,L,L), 1 where the chain evolves; x_initial: device fp32; both NULL = unconditional */
int t2p_sampler_set_condition(t2p_sampler* s, const uint8_t* mask, const float* x_initial);
/* Classifier-free guidance in the PC loop (reference sampler/diffusion_sampler.py:128, a property of the network output: the
 * reference's pc_sampler takes it as a wrapper module).  Enabled, every score of the loop is w out(ctx) + (1 - w) out(0), from ONE
 * evaluation per score of [x ; x] under [ctx ; 0] at batch 2B; the sum (and, VP, the score scale) is formed inside the norm and
 * update kernels.  w == 1 runs the plain path at batch B, as the DDIM loop does.  A non-finite w is refused and nothing changes.
 * May be called between runs; drops a captured graph.  The context has to be set (again) afterwards: t2p_sampler_set_context. */
int t2p_sampler_set_guidance(t2p_sampler* s, double w, int enabled);
/* context: device fp32 [batch][tokens][context_dim].  Guided with w != 1: builds [ctx ; 0] on the device and projects it through
 * the engine at batch 2B; otherwise forwards to t2p_engine_set_context at batch B.  batch != cfg.batch is refused, nothing changes.
 * A guided step without it is refused. */
int t2p_sampler_set_context(t2p_sampler* s, const float* context, int batch, int tokens, void* stream);
/* Replacement inpainting (reference score_sde_pytorch/inpainting.py, get_pc_inpainter): fixes a motif for a network that was NOT
 * trained under the `inpainting` condition.  After every corrector update (its last inner Langevin step) and every predictor update
 * of loop step i the known region is overwritten with the data noised to that level,
 *     r = fl(fl(mean_coef[i] data) + fl(z std[i])),   x = known ? r : x,   x_mean = known ? fl(mean_coef[i] data) : x
 * (off the known region x_mean is the NEW x, not the update's mean: inpainting.py:46).  This happens inside the update kernels:
 * a step enqueues the same number of dispatches with and without it.  known: device uint8 (B,C,L,L), 1 = known (the reference's
 * mask); data: device fp32 (B,C,L,L); both borrowed.  mean_coef / std: HOST tables of N floats, (a_i, s_i) of
 * sde.marginal_prob(data, t_i), t = linspace(T, eps, N) (VE: a_i == 1), copied.  All four NULL clears the replacement; tables
 * without pointers or pointers without tables are refused and nothing changes.  Under a condition (t2p_sampler_set_condition) the
 * precedence per element is: frozen by the condition -> x_initial; else known -> replaced; else the update.  Under guidance both
 * halves of x receive the replaced state.  t2p_sampler_run with prior_given == 0 starts from known ? data : prior.
 * z is drawn inside the kernels (Philox streams 0x80000000 after the corrector, 0x80000001 after the predictor; step word = loop
 * step) unless t2p_sampler_set_inpaint_noise gives device draws (B,C,L,L) for the following steps (fixture replay; NULL = device
 * draws again).  Injected corrector-side noise with n_steps_each > 1 is refused, as in t2p_sampler_step; a captured step
 * (t2p_sampler_step_graph) refuses injected noise and re-captures when known / data change. */
int t2p_sampler_set_inpaint(t2p_sampler* s, const uint8_t* known, const float* data, const float* mean_coef, const float* std);
int t2p_sampler_set_inpaint_noise(t2p_sampler* s, const float* after_corrector, const float* after_predictor);
/* reset the step counter to `step` (0 at the start of a run) for a fresh x; a step at index >= N is refused */
int t2p_sampler_reset(t2p_sampler* s, int step, void* stream);
/* One PC step at the current step index, in place on x (device fp32 (B,C,L,L)); x_mean receives the
 * predictor's mean.  noise_corrector / noise_predictor: device standard-normal draws to use
 * (parity runs); NULL = generate on device.
 * Guided with w != 1 (t2p_sampler_set_guidance), here and in t2p_sampler_step_graph / _run / _count_dispatches: the state is the
 * first (B,C,L,L) block of x and x must have room for 2B samples: the second block is the sampler's copy of the first (the [x ; x]
 * input), written by the first step after t2p_sampler_reset and by every update.  x_mean and the noise stay (B,C,L,L). */
int t2p_sampler_step(t2p_sampler* s, float* x, float* x_mean, const float* noise_corrector,
                     const float* noise_predictor, void* stream);
/* The same step replayed from a captured hipGraph (on-device noise only).  The first call runs
 * eagerly (it sizes the activation pool), the second captures, later calls replay; x / x_mean /
 * the condition pointers must stay the same between calls (a change triggers a re-capture).
 * `stream` must be a real stream (capture on the NULL stream is not allowed). */
int t2p_sampler_step_graph(t2p_sampler* s, float* x, float* x_mean, void* stream);
/* Full run: x must hold the (already conditioned) prior sample on entry when `prior_given`, else it
 * is drawn on device (randn * sigma_max, then mask applied).  out receives x_mean (denoise) or x. */
int t2p_sampler_run(t2p_sampler* s, float* x, float* out, int prior_given, int n_steps, void* stream);
/* measurement: the number of device dispatches (graph nodes) one PC step (sampling.py:279-285) enqueues; the step is captured
 * on `stream` (not the default stream) and discarded, nothing executes; call after at least one eager step */
int t2p_sampler_count_dispatches(t2p_sampler* s, float* x, float* x_mean, void* stream, int* n_out);

/* ---- DDIM sampler with classifier-free guidance ---------------------------------------------------
 * The reference's second sampler for the same network (sampler/diffusion_sampler.py, twin model/diffusion_sampler.py): a strided
 * DDIM loop over a VP-trained noise predictor, guided on the text embedding, with static clipping of the predicted clean sample.
 * t2p_ddim_create        <- DiffusionSampler.__init__ + the schedule of ddim_sample        (diffusion_sampler.py:13-64, 87-89)
 * t2p_ddim_set_context   <- `cond` and `cond * 0`                                          (:128)
 * t2p_ddim_step          <- one iteration of the loop body                                 (:94-112, 116-142)
 * t2p_ddim_run           <- ddim_sample(shape, cond)                                       (:72-114)
 * Guidance costs ONE evaluation per step: the context is [ctx ; 0] at batch 2B (to_k / to_v have no bias, so the zero half gives
 * zero keys and values, as `cond * 0` does) and the network runs on [x ; x].  With w == 1 the zero-context half is skipped
 * (batch B): 1 a + 0 b == a for finite b -- the one place the evaluation count differs from the reference, which evaluates both. */
typedef struct t2p_ddim_config {
  int32_t timesteps;        /* length of the beta schedule; labels are < timesteps <= model.num_scales   */
  int32_t sampling_steps;   /* rows of the step table                                                     */
  double eta;               /* ddim_eta in [0, 1]                                                         */
  double w;                 /* guidance weight: eps = w eps(ctx) + (1 - w) eps(0)                         */
  int32_t clip;             /* 1 = clamp the predicted clean sample to [-1, 1] ('static'), 0 = 'dynamic' */
  int32_t batch;            /* chains B                                                                   */
  uint64_t seed;            /* on-device Philox noise: draw 0 is the prior, draw k + 1 belongs to step k  */
} t2p_ddim_config;
/* one loop step (t, t_next) of ddim_sample, in the reference's float32 arithmetic: t the time label; sqrt_recip / sqrt_recipm1 =
 * sqrt_recip(m1)_alphas_cumprod[t]; sqrt_an = sqrt(alphas_cumprod[t_next]); c, sigma as :105-106; last = (t_next < 0): the step
 * returns the clean sample and reads no noise (the other three are then ignored) */
typedef struct t2p_ddim_step_row {
  int32_t t;
  float sqrt_recip, sqrt_recipm1, sqrt_an, c, sigma;
  int32_t last;
} t2p_ddim_step_row;
typedef struct t2p_ddim t2p_ddim;
/* table: host rows [cfg->sampling_steps], copied.  Refused with nothing created: an engine that is not finalized, eta outside
 * [0, 1], sampling_steps < 1, a label outside [0, num_scales), timesteps outside [1, num_scales], batch < 1. */
int t2p_ddim_create(t2p_engine* e, const t2p_ddim_config* cfg, const t2p_ddim_step_row* table, t2p_ddim** out);
void t2p_ddim_destroy(t2p_ddim* d);
int t2p_ddim_set_seed(t2p_ddim* d, uint64_t seed);
/* mask: device uint8 (B,C,L,L), 1 where the chain evolves; x_initial: device fp32; both NULL = unconditional.  Frozen entries are
 * re-imposed by every update (an extension: the reference's DDIM loop takes no condition).  The pointers are borrowed. */
int t2p_ddim_set_condition(t2p_ddim* d, const uint8_t* mask, const float* x_initial);
/* context: device fp32 [batch][tokens][context_dim]; builds [ctx ; 0] on the device and projects it through the engine
 * (t2p_engine_set_context at batch 2B; at batch B when w == 1).  batch != cfg.batch is refused, nothing changes. */
int t2p_ddim_set_context(t2p_ddim* d, const float* context, int batch, int tokens, void* stream);
/* the next t2p_ddim_step is loop step `step` (0 at the start of a run) on a fresh x; a step outside the table is refused */
int t2p_ddim_reset(t2p_ddim* d, int step, void* stream);
/* One DDIM step at the current step index, in place on x (device fp32; the state is its first (B,C,L,L) block).  With w != 1, x
 * must have room for 2B samples: the second block is the engine's copy of the first (the [x ; x] input), written by the first step
 * after t2p_ddim_reset and by every update.  x0_out (optional): device fp32 (B,C,L,L), the clipped clean-sample prediction.
 * noise: device standard-normal draws (parity runs) or NULL = drawn inside the update kernel.  Enqueues on `stream` only: no host
 * synchronisation, copy or allocation once the first step has sized the engine's activation pool.  A step beyond the table is
 * refused and x is left unchanged. */
int t2p_ddim_step(t2p_ddim* d, float* x, float* x0_out, const float* noise, void* stream);
/* Full run: x (sized as for t2p_ddim_step) holds the already conditioned prior when `prior_given`, else it is drawn on the device
 * (randn, then the mask); n_steps <= 0 = the whole table.  out: device fp32 (B,C,L,L), may be x. */
int t2p_ddim_run(t2p_ddim* d, float* x, float* out, int prior_given, int n_steps, void* stream);
/* The update of one DDIM step as an operator over n elements, every scalar by value:
 *   eps = w eps_c + w1 eps_u   (eps_u NULL: eps = eps_c; w1 = (float)(1 - w) as the reference rounds it)
 *   x0 = sqrt_recip x - sqrt_recipm1 eps, clamped to [-1, 1] when clip;   x_next = last ? x0 : x0 sqrt_an + c eps + sigma z
 *   x_next = mask ? x_next : x_initial
 * each product and sum rounded to float32 in this order.  z NULL = drawn in the kernel, equal to t2p_op_philox_normal(seed,
 * stream_id) bit for bit (nothing is drawn when sigma == 0); no z is read or drawn when last.  x_out may alias x; x_out2
 * (optional) receives a second copy of x_next, x0_out (optional) the clean-sample prediction. */
int t2p_op_ddim_update(const float* x, const float* eps_c, const float* eps_u, const float* z, const uint8_t* mask,
                       const float* x_initial, float* x_out, float* x_out2, float* x0_out, int64_t n, float w, float w1,
                       float sqrt_recip, float sqrt_recipm1, float sqrt_an, float c, float sigma, int clip, int last,
                       uint64_t seed, uint64_t stream_id, void* stream);

/* ---- training step ---------------------------------------------------------------
 * model->compute_dtype selects the products: T2P_DTYPE_F32 exact f32; T2P_DTYPE_F16 / T2P_DTYPE_BF16 16-bit operands with fp32
 * accumulation (residual-block 3x3 convolutions on the 16-bit implicit GEMM, every other product on t2p_op_tgemm16; input / head
 * convolutions, norms, softmax and elementwise work stay fp32).  Parameters, gradients, Adam moments, EMA and loss are fp32 in every
 * mode.  The objective is the denoising score-matching loss under the VE (default), VP or sub-VP SDE (t2p_train_set_sde), or the DDIM
 * sampler's noise-prediction loss (t2p_train_set_ploss).  16-bit modes seed the backward pass with S dL/do (S = 2^round(log2(B C L L)),
 * or a power of two chosen on the device where the seed carries 1 / sigma) and divide S out of the gradient buffer, so
 * t2p_train_read(GRAD) and t2p_train_grad_buffer hold true gradients; every reduction that feeds a gradient or an update runs in a
 * fixed order (gradients and post-step state bitwise reproducible; the scalar loss is summed with double atomics), and
 * t2p_train_step / t2p_train_apply return an error and change nothing (parameters, moments, EMA, counters) when the loss or the
 * gradient norm is not finite.
 * t2p_train_create      <- get_model + get_optimizer + ExponentialMovingAverage(model.parameters(), decay)
 *                          (score_sde_pytorch/utils.py:4-9, losses.py:26-36, models/ema.py:13-30; train.py builds `state` from them)
 * t2p_train_set_sde     <- the `sde` of get_sde_loss_fn / get_step_fn (losses.py:66,140): VE (the default), VP or sub-VP
 * t2p_train_set_ploss   <- DiffusionSampler.p_loss / forward (sampler/diffusion_sampler.py:144-167) as the objective instead of an SDE loss:
 *                          integer timesteps, the sampler's own sqrt_alpha_cumprod tables, l1 or l2 on the predicted noise
 * t2p_train_load_param  <- load_state_dict of one tensor; the EMA shadow starts as a copy (ema.py:28-29)
 * t2p_train_loss        <- loss_fn(model, batch, condition)      (losses.py:105-134), optionally with loss.backward()
 * t2p_train_step        <- step_fn(state, batch, condition), train=True (losses.py:165-176): zero_grad, loss, backward,
 *                          optimize_fn (warm-up on state['step'], clip_grad_norm_, Adam: losses.py:41-49), step += 1, ema.update
 * t2p_train_eval_loss   <- step_fn with train=False (losses.py:177-183): the loss under the EMA weights, model in eval mode
 * t2p_train_set_ss_blocks <- block_dropout(coords_6d, batch["ss_indices"]) under the ss condition (losses.py:54-64, called at :106-107)
 * t2p_train_set_inpaint_draw <- utils.random_mask_batch(batch, config) (utils.py:15-60), which train.py calls before every train and eval
 *                          step (train.py:176, :193) when "inpainting" is in the condition
 * t2p_train_set_context_drop <- (no counterpart: the reference's loss has no context dropout) per-sample dropout of the text context,
 *                          the training that gives the guided samplers' out(context * 0) a meaning
 * The model runs in train mode (models/utils.py:116-118): Dropout_0 of every residual block is active when dropout > 0.       */
typedef struct t2p_train_config {
  double lr, beta1, eps, weight_decay;   /* optim.lr / beta1 / eps / weight_decay; beta2 = 0.999 as get_optimizer fixes it    */
  double warmup;                          /* optim.warmup: lr * min(step / warmup, 1) when > 0                                   */
  double grad_clip;                       /* optim.grad_clip: clip_grad_norm_(max_norm) when >= 0                                */
  double ema_rate;                        /* model.ema_rate                                                                      */
  double dropout;                         /* model.dropout (Dropout_0 of ResnetBlockBigGANpp, layers.py:293,318)                 */
  double t_eps;                           /* smallest time drawn, 1e-5 (get_sde_loss_fn's eps)                                   */
  int32_t cond_flags;                     /* model.condition: 1 length | 2 ss | 4 inpainting (losses.py:113-123)                */
  uint64_t seed;                          /* on-device draws of t, z and the dropout masks when the batch does not supply them   */
} t2p_train_config;

typedef struct t2p_train_batch {
  const float* coords_6d;      /* device fp32 (batch, C, L, L): batch["coords_6d"]                                               */
  const uint8_t* mask_pair;    /* device uint8 (batch, L, L):   batch["mask_pair"]                                               */
  const uint8_t* mask_inpaint; /* device uint8 (batch, L, L):   batch["mask_inpaint"], needed with the inpainting condition      */
  const float* context;        /* device fp32 (batch, tokens, context_dim): llm.model.embed_tokens(caption tokens)              */
  int32_t batch, tokens;
  const float* t;              /* device fp32 [batch] or NULL = t ~ U(t_eps, 1) drawn on the device (losses.py:106); under          */
                               /* t2p_train_set_ploss: the integer timesteps as floats, NULL = drawn in [0, timesteps)           */
  const float* z;              /* device fp32 (batch, C, L, L) or NULL = z ~ N(0, 1) drawn on the device (losses.py:107)         */
} t2p_train_batch;

typedef struct t2p_trainer t2p_trainer;
int t2p_train_create(const t2p_model_config* model, const t2p_train_config* train, t2p_trainer** out);
void t2p_train_destroy(t2p_trainer* t);
int t2p_train_num_params(const t2p_trainer* t);
/* name and shape of tensor i in the reference's parameters() order (the order of the EMA shadow list and of the optimizer state) */
int t2p_train_param_info(const t2p_trainer* t, int i, const char** name, int64_t shape[4], int* ndim);
int t2p_train_load_param(t2p_trainer* t, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* which: 0 parameter, 1 gradient of the last backward pass (after t2p_train_step: as clip_grad_norm_ left it), 2 EMA shadow,
 * 3 Adam exp_avg, 4 Adam exp_avg_sq; host buffers of the tensor's size, reference layout */
int t2p_train_read(t2p_trainer* t, int which, const char* name, float* host_out);
int t2p_train_write(t2p_trainer* t, int which, const char* name, const float* host_in);
/* state['step'] (drives the warm-up), the optimizer's own update count (Adam bias correction) and ema.num_updates */
int t2p_train_set_step(t2p_trainer* t, int64_t step, int64_t adam_updates, int64_t ema_updates);
int t2p_train_get_step(const t2p_trainer* t, int64_t out3[3]);
/* SDE of the loss (get_sde_loss_fn's `sde`, losses.py:66): T2P_SDE_VE (the default after create), T2P_SDE_VP or T2P_SDE_SUBVP.
 * Call after t2p_train_create and before the first loss.  VE: std = sigma_min (sigma_max / sigma_min)^t, mean = x, integer label
 * round((1 - t)(N - 1)).  VP / sub-VP (sde_lib.py:134-138, 184-188; models/utils.py:138-157): mean = exp(lmc) x, std = sqrt(1 - exp(2 lmc))
 * resp. 1 - exp(2 lmc), the network receives the float label t (N - 1) resp. 999 t and its output o becomes the score
 * -o / sqrt_1m_alphas_cumprod[trunc(label)] resp. -o / std.  beta_min / beta_max: ignored for VE but checked.
 * std_table: VP only, host float[num_scales] = sde.sqrt_1m_alphas_cumprod as the reference builds it in float32 (sde_lib.py:118-122);
 * NULL otherwise.  Refused with nothing changed: an unknown sde; beta_max <= beta_min or beta_min <= 0; VP without a table; sub-VP with
 * scale_by_sigma and num_scales < 1000 (the reference would index sigmas[trunc(999 t)] out of range). */
int t2p_train_set_sde(t2p_trainer* t, int sde, double beta_min, double beta_max, const float* std_table);
/* The DDIM sampler's training objective (sampler/diffusion_sampler.py:144-167: q_sample, p_loss, forward) instead of an SDE loss.
 * loss_type: 1 = l1, 2 = l2.  The two tables are host float[timesteps] (DiffusionSampler's sqrt_alpha_cumprod and
 * sqrt_one_minus_alphas_cumprod, built in float32 from whatever betas it was given) and are copied; timesteps is not tied to
 * num_scales.  Call after t2p_train_create and before the first pass; the trainer keeps the objective.  Every pass then computes
 *   t_b      batch->t[b] (device fp32 holding the integer timestep, exact below 2^24; the table index is clamped to [0, timesteps - 1],
 *            range and integrality are the caller's to check), or with batch->t NULL drawn on the device: t_b = ((w >> 8) timesteps) >> 24,
 *            w = word 0 of Philox4x32-10 under the trainer seed, training layout, counter b, stream 4096 loss_calls + 5 (csrc/philox.h)
 *   x_noisy  sqrt_alphas_cumprod[t_b] x + sqrt_one_minus_alphas_cumprod[t_b] z  (:147-148; the product and sum of the VP step's kernel)
 *   o        UNetModel.forward on (x_noisy, the INTEGER label t_b, context), train mode (Dropout_0 active) -- or eval mode under the EMA
 *            in t2p_train_eval_loss -- with that method's own h / sigmas[t_b] when scale_by_sigma is set (ncsnpp.py:259-261; no SDE
 *            conversion follows); score_out receives o (NCHW), the predicted noise
 *   loss     r = o - z.  batch->mask_pair NULL: the reference's loss, mean |r| or mean r^2 over EVERY element (:156-159; padding included,
 *            cond_flags ignored, nothing frozen; mask_inpaint is not read).  batch->mask_pair given (an extension, as `condition` in the
 *            DDIM sampler: frozen entries stay clean in training as the sampler re-imposes them): the mask of the SDE loss (mask_pair x
 *            the conditional mask of cond_flags, mask_inpaint, the drawn inpainting mask), x_noisy = where(mask, x_noisy, x), per sample
 *            sum_mask |r| or r^2 over (num_elem + 1e-8), then the mean over samples (the form of losses.py:128-131: equal shards under data
 *            parallelism reproduce the whole batch); ss block dropout is honoured.
 * Context dropout, t2p_train_eval_loss, t2p_train_apply, the gradient buffer and t2p_train_copy work unchanged.  16-bit modes seed the
 * backward pass with the host power of two S of the VE step (l1 seeds are +-S / ((num_elem + 1e-8) batch)) -- except under
 * scale_by_sigma, where residual and seed carry 1 / sigmas[t_b] (up to 1 / sigma_min) and S is chosen on the device as under VP.
 * Refused with nothing changed: after t2p_train_set_sde to VP or sub-VP; after a pass has run; a second call; a loss_type other than
 * 1 or 2; timesteps < 1 or > 2^24; a NULL table; with scale_by_sigma, timesteps > num_scales (the reference would index sigmas out of
 * range).  Afterwards every t2p_train_set_sde is refused.  The unmasked pass with a pending ss
 * block list or inpaint-draw request returns an error, computes and changes nothing, and the request is cleared. */
int t2p_train_set_ploss(t2p_trainer* t, int loss_type, int timesteps, const float* sqrt_alphas_cumprod,
                        const float* sqrt_one_minus_alphas_cumprod);
/* parity runs: keep-masks of Dropout_0 for the next pass, one device uint8 [batch][H][W][C] (NHWC, the block's own resolution and
 * width) per residual block in forward order; n = 0 returns to on-device Philox masks */
int t2p_train_set_dropout_masks(t2p_trainer* t, const uint8_t* const* device_masks, int n);
/* block_dropout (losses.py:54-64, called at :106-107 when "ss" is in the condition): every secondary-structure block of every sample
 * is dropped with probability p (the reference: 0.2); a dropped block zeroes channels 4:7 on its rows start:end and on its columns
 * start:end.  host_blocks: host int32 [n][3] = (sample, start, end), end exclusive, Python slice semantics on an axis of length L (end
 * clamped to L, start >= end empty, overlapping blocks fine).  host_drop: host uint8 [n], the decision per block (parity runs, or draws
 * made by the caller in the reference's order), or NULL = drawn on the device: block k is dropped iff u < (float)p, u one Philox
 * uniform keyed by the trainer seed (counter k, a stream of its own per loss call).  Both arrays are copied at the call.  The list is
 * per-batch data: the NEXT t2p_train_loss / t2p_train_step / t2p_train_eval_loss consumes it (the reference applies the dropout with
 * train=False too) and clears it; n = 0 clears it.  The reference zeroes its coords_6d argument in place; here batch->coords_6d is
 * NOT modified, the zeroing happens on the way into the perturbed input (both branches of losses.py:129's torch.where see it).
 * Refused with nothing changed: n > 0 on a trainer whose cond_flags lacks bit 2; p outside [0, 1]; a negative start or end (not
 * wrapped: the dataset never writes one); sample < 0.  A sample >= batch shows at the pass: that pass returns an error, computes and
 * changes nothing, and the list is cleared. */
int t2p_train_set_ss_blocks(t2p_trainer* t, const int32_t* host_blocks, int n, const uint8_t* host_drop, double p);
/* random_mask_batch (utils.py:15-60; train.py:176, :193): the random inpainting mask of a batch that supplies none, drawn on the device.
 * host_len_lo_hi: host int32 [B][3] = (l, lo, hi) per sample -- l valid residues, lo = int(mask_min_len l), hi = int(mask_max_len l),
 * both products in double as Python forms them; copied at the call.  One uniform u0 per batch picks the mode: a random subset when
 * u0 < (float)random_p, a contiguous window when u0 > (float)(1.0 - contiguous_p), else none (every residue flagged, the padding
 * included: mask_pair removes it).  Per sample r = lo + (((w0 >> 8) (hi - lo)) >> 24) residues in [lo, hi) are flagged: the window
 * start .. start + r with start = ((w1 >> 8) (l - r)) >> 24, or the r residues whose 32-bit keys rank lowest among the l valid ones (ties
 * to the lower index: exactly r, every subset of that size equally likely).  mask_inpaint[b][i][j] = flag[b][i] | flag[b][j]; r = 0
 * (lo = 0) flags nothing, that sample's num_elem is 0 and its loss term 0 / 1e-8 = 0.  All words are Philox4x32-10 under the trainer seed
 * on a stream of its own per loss call (csrc/philox.h tabulates the counters), so the draws differ from torch's; the distribution is
 * the reference's except that r and start come from 24-bit words.
 * Per-batch data, like the ss block list: the NEXT t2p_train_loss / t2p_train_step / t2p_train_eval_loss whose batch->mask_inpaint is
 * NULL draws into a trainer-owned buffer that goes where batch->mask_inpaint goes, and consumes the request; a pass whose batch
 * supplies mask_inpaint ignores the request and clears it; B = 0 clears it.  Refused with nothing changed (a request set earlier
 * stays): a trainer whose cond_flags lacks bit 4 or whose max_res_num exceeds 256; a probability outside [0, 1] or a sum above 1;
 * l < 0 or l > max_res_num; lo < 0, lo >= hi or hi > l for any sample (torch.randint raises on the empty range, e.g. l = 1).  A B that
 * differs from the pass's batch fails that pass, which computes and changes nothing, and the request is cleared.  Without a request
 * and without mask_inpaint the pass is refused as before ("the inpainting condition needs batch.mask_inpaint"). */
int t2p_train_set_inpaint_draw(t2p_trainer* t, const int32_t* host_len_lo_hi, int B, double random_p, double contiguous_p);
/* Text-context dropout, the training side of classifier-free guidance (the samplers evaluate w out(ctx) + (1 - w) out(ctx * 0); the
 * second term needs a network that has trained on an all-zero context).  Every sample b of the batch is dropped independently; a dropped
 * sample trains exactly as if batch->context[b] were all zeros; kept samples and batch->context itself are not touched.  host_drop: host
 * uint8 [B], the decision per sample (copied at the call), or NULL with B > 0 = drawn on the device: sample b is dropped iff
 * u < (float)p, u one Philox uniform keyed by the trainer seed (training layout, counter b, stream 4096 loss_calls + 4: csrc/philox.h).
 * attn2.to_k and attn2.to_v have no bias, so a zero context is K = V = 0: the pass zeroes the dropped samples' rows of every projected
 * K and V in place (no copy of the context) and, in the backward pass, the same rows of dK and dV before the projections' weight
 * gradients are formed -- those receive nothing from a dropped sample.
 * Per-batch data, like the ss block list: the NEXT t2p_train_loss / t2p_train_step / t2p_train_eval_loss consumes the request,
 * whatever becomes of that pass (eval_loss after explicit all-ones decisions is the unconditional evaluation loss); B = 0 clears it.
 * A pass without a request makes no launch and no draw for this.  Refused, leaving the stored request as it was: B < 0; p outside
 * [0, 1] or NaN.  A B that differs from the pass's batch fails that pass, which computes and changes nothing, and the request is cleared. */
int t2p_train_set_context_drop(t2p_trainer* t, const uint8_t* host_drop, int B, double p);
/* loss_host: host float; score_out (optional): device fp32 (batch, C, L, L), the score the loss was computed from */
int t2p_train_loss(t2p_trainer* t, const t2p_train_batch* batch, int backward, float* loss_host, float* score_out, void* stream);
int t2p_train_step(t2p_trainer* t, const t2p_train_batch* batch, float* loss_host, void* stream);
/* Data-parallel training (the reference wraps the model in DataParallel, score_sde_pytorch/utils.py:8: one gradient over the whole
 * batch): every process runs t2p_train_loss(backward = 1) on its shard, the flat gradient buffer (device fp32 [n], parameters() order,
 * owned by the trainer) is averaged over the processes -- ONE RCCL all-reduce -- and t2p_train_apply runs optimize_fn + step += 1 +
 * ema.update on it.  t2p_train_step = t2p_train_loss(backward = 1) + t2p_train_apply. */
int t2p_train_grad_buffer(t2p_trainer* t, float** device_ptr, int64_t* n);
int t2p_train_apply(t2p_trainer* t, void* stream);
/* The flat fp32 device buffers (parameters() order, owned by the trainer): which = 0 parameters, 2 EMA shadow (t2p_train_read's numbers) */
int t2p_train_buffer(t2p_trainer* t, int which, float** device_ptr, int64_t* n);
/* ema.store / ema.copy_to / ema.restore (models/ema.py:51-84) as device-to-device copies of the flat buffers on `stream`: dst <- src is
 * exactly one of 5 <- 0 (store: 5 is a stash, allocated by the first store and counted in t2p_train_device_bytes), 0 <- 2 (copy_to) or
 * 0 <- 5 (restore; refused before any store).  A copy into the parameters also renews the trainer's kernel-layout weight copies. */
int t2p_train_copy(t2p_trainer* t, int dst, int src, void* stream);
/* t2p_train_buffer + t2p_engine_load_flat: the sampling engine takes the trainer's parameters (which = 0) or EMA (2) without leaving the
 * device; the compute dtypes of the two may differ.  Refused with nothing changed (the engine keeps its weights and still scores), each
 * with its own message: parameter tables that differ in count, a name or a shape; different devices; any other `which`. */
int t2p_engine_load_from_trainer(t2p_engine* e, t2p_trainer* t, int which, void* stream);
int t2p_train_eval_loss(t2p_trainer* t, const t2p_train_batch* batch, float* loss_host, void* stream);
int64_t t2p_train_device_bytes(const t2p_trainer* t);
/* the strided fp32 GEMM of the backward pass: C[z][m][n] = alpha sum_k A(z,m,k) B(z,k,n) + beta C, element strides as given
 * (one stride of each operand must be 1); conv = 1: B is the 3x3 window gather of the NHWC map X [batch][H][W][conv_C] (weight
 * gradient of a convolution: K = batch H W, N = 9 conv_C, sBk/sBn ignored, ldx = sBz0); ksplit 0 = chosen by the library (needs beta = 1 when > 1) */
int t2p_op_tgemm(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc, int M, int N,
                 int K, int nz, int64_t sAz, int64_t sBz, int64_t sCz, float alpha, float beta, const float* bias_n, int ksplit, int conv,
                 int H, int W, int conv_C, void* stream);
/* the same product on the 16-bit matrix pipe (dtype 1 = bf16, 2 = f16; the mixed-precision training step): A, B, C and bias stay fp32 in
 * memory, A and B are rounded to dtype (nearest even, no saturation: an overflow becomes +-inf) as they are staged, products accumulate
 * in fp32; split-K sums its partial tiles in a fixed order (bitwise reproducible, any beta).  Same arguments as t2p_op_tgemm. */
int t2p_op_tgemm16(int dtype, const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C, int64_t ldc,
                   int M, int N, int K, int nz, int64_t sAz, int64_t sBz, int64_t sCz, float alpha, float beta, const float* bias_n, int ksplit,
                   int conv, int H, int W, int conv_C, void* stream);
/* one 3x3 convolution of the training step (nn.Conv2d, padding 1, + the per-sample time-embedding bias of layers.py:316), forward and
 * backward, through the code the trainer runs (train.h: train_conv3x3_forward / train_conv3x3_backward) in the trainer's order: the
 * weight layouts (conv_w_prep) and, for dtype 1 = bf16 / 2 = f16, their 16-bit copies and those of x / dy as HipTrainModel(dtype=...)
 * makes them for a residual-block convolution (dtype 0: the exact-f32 kernels, which the input and head convolutions keep in every
 * mode); the forward product; the data gradient in place; the gathered weight gradient with the library's split-K; its fold into the
 * reference layout; the column sums.  All pointers device fp32:
 *   x [batch][H W][Cip] NHWC, pad columns zero;  w [Co][Ci][3][3];  bias [Co];  tbias [batch][Co] or NULL (needs Cop == Co)
 *   y [batch][H W][Cop]: Co columns written, the pad columns zeroed
 *   dy [batch][H W][Cop]; NULL = forward only.   dx [batch][H W][Cip], ACCUMULATED into (Ci columns; the pad columns untouched);
 *   NULL = x needs no gradient.   dw [Co][Ci][3][3], dbias [Co], dtbias [batch][Co] (with tbias): ACCUMULATED into
 * fixed_order: the reductions of the 16-bit step (column sums in a fixed order; plan switch 48's meaning), else atomics.
 * Cip, Cop: multiples of 4 (of 8 for dtype 1 / 2), >= Ci, Co.  Scratch is allocated inside the call and freed before it returns. */
int t2p_op_train_conv3x3(int dtype, const float* x, const float* w, const float* bias, const float* tbias, int batch, int H, int W, int Ci,
                         int Co, int Cip, int Cop, float* y, const float* dy, float* dx, float* dw, float* dbias, float* dtbias,
                         int fixed_order, void* stream);
/* block_dropout alone (losses.py:54-64; the training pass applies it at :106-107 through the same two kernels): out = x (device fp32
 * (batch, C, L, L)) with channels 4:7 of the dropped blocks' rows and columns zeroed; out may alias x, otherwise x is untouched.
 * host_blocks / host_drop / p as t2p_train_set_ss_blocks; seed / stream_id: the Philox key and stream of the device draws (host_drop
 * NULL); drop_out_device (optional): device uint8 [n], the decisions used.  Refused: C < 7, a negative start or end, a sample outside
 * [0, batch), p outside [0, 1]. */
int t2p_op_ss_block_dropout(const float* x, float* out, int batch, int C, int L, const int32_t* host_blocks, int n,
                            const uint8_t* host_drop, double p, uint64_t seed, uint64_t stream_id, uint8_t* drop_out_device, void* stream);
/* the draw of t2p_train_set_inpaint_draw alone, through the same kernel: flags_out device uint8 [B][L] (1 = residue masked), pair_out
 * device uint8 [B][L][L] = flags[b][i] | flags[b][j], mode_out_host (optional) host int = the mode used (0 none, 1 random, 2 contiguous).
 * seed / stream_id: the Philox key and stream (the trainer's: its seed and 4096 loss_calls + 3).  force_mode: -1 = drawn from u0,
 * 0 / 1 / 2 = that mode with the per-sample words unchanged.  L <= 256.  Refused with the outputs untouched: what
 * t2p_train_set_inpaint_draw refuses (with L for max_res_num), B <= 0, a force_mode outside -1 .. 2. */
int t2p_op_inpaint_mask_draw(const int32_t* host_len_lo_hi, int B, int L, double random_p, double contiguous_p, uint64_t seed, uint64_t stream_id,
                             int force_mode, uint8_t* flags_out, uint8_t* pair_out, int* mode_out_host, void* stream);
/* the timestep draw of t2p_train_set_ploss alone, through the same device function: out_dev device int32 [B], out_dev[b] =
 * ((w >> 8) timesteps) >> 24 with w = word 0 of the Philox block (key seed, training layout, counter b, stream stream_id; the trainer's:
 * its seed and 4096 loss_calls + 5).  Refused: B <= 0, timesteps outside [1, 2^24], a NULL output. */
int t2p_op_ploss_draw_t(uint64_t seed, uint64_t stream_id, int B, int timesteps, int32_t* out_dev, void* stream);
/* the two kernels of t2p_train_set_context_drop alone, in place on x = device fp32 [batch][row_floats] (16-byte aligned): the decisions
 * (host_drop: host uint8 [batch], or NULL = drawn at probability p under the Philox key `seed` and stream `stream_id`, the trainer's:
 * its seed and 4096 loss_calls + 4), then row b of x becomes +0.0f where sample b is dropped -- stored, not multiplied, so an Inf or a
 * NaN becomes 0; the other rows are neither read nor written.  drop_out_device (optional): device uint8 [batch], the decisions used.
 * Refused with x untouched: batch <= 0, row_floats <= 0 or not a multiple of 4 (16-byte stores), p outside [0, 1]. */
int t2p_op_context_drop(float* x, int batch, int64_t row_floats, const uint8_t* host_drop, double p, uint64_t seed, uint64_t stream_id,
                        uint8_t* drop_out_device, void* stream);
/* backward halves of the operators (gradients accumulate into dx / dgamma / dbeta / du) */
int t2p_op_groupnorm_backward(const float* x, const float* dy, const float* gamma, const float* beta, int silu, int batch, int HW, int C,
                              int groups, float eps, float* dx, float* dgamma, float* dbeta, void* stream);
int t2p_op_layernorm_backward(const float* x, const float* dy, const float* gamma, int64_t rows, int C, float eps, float* dx, float* dgamma,
                              float* dbeta, void* stream);
/* the same with the form of the parameter-gradient reduction chosen by the caller: fixed_order = 0 float atomics (the f32 step, what the
 * two entries above run), 1 a fixed summation order through a workspace the call allocates and frees (what the 16-bit step runs:
 * bitwise reproducible) */
int t2p_op_groupnorm_backward_form(const float* x, const float* dy, const float* gamma, const float* beta, int silu, int batch, int HW,
                                   int C, int groups, float eps, float* dx, float* dgamma, float* dbeta, int fixed_order, void* stream);
int t2p_op_layernorm_backward_form(const float* x, const float* dy, const float* gamma, int64_t rows, int C, float eps, float* dx,
                                   float* dgamma, float* dbeta, int fixed_order, void* stream);
/* column sums (bias gradients; nz = batch: the per-sample time-embedding bias): out[z][n] (+)= sum_r dy[(z rows_per_z + r) ld + n],
 * n < N, out rows of ld_out floats (columns N.. untouched); accumulate = 0 overwrites; fixed_order as above */
int t2p_op_colsum(const float* dy, int nz, int64_t rows_per_z, int N, int64_t ld, float* out, int64_t ld_out, int accumulate,
                  int fixed_order, void* stream);
/* *result_host = sum g[i]^2 in double (the gradient norm of clip_grad_norm_ and of the overflow guard); fixed_order as above */
int t2p_op_sumsq(const float* g, int64_t n, int fixed_order, double* result_host, void* stream);
/* the backward seed's scale of the 16-bit VP / sub-VP step: s2_host[0] = S = 2^e, e = the largest integer with 2^e max|x| <= target,
 * clamped to [-60, 60] (so S and 1 / S are normal floats whatever x holds, a subnormal maximum included); S = 1 when x is all zero
 * or holds an infinity or a NaN; s2_host[1] = 1 / S.  target > 0 */
int t2p_op_seed_scale(const float* x, int64_t n, float target, float* s2_host, void* stream);
int t2p_op_softmax_backward(const float* P, float* dP_inout, int64_t rows, int n, float scale, void* stream);
int t2p_op_geglu_backward(const float* u, const float* dy, float* du, int64_t rows, int inner, void* stream);

/* ---- individual operators (parity tests call these through the same ABI) -------------------- */
int t2p_op_gemm(int dtype, const void* A, int a_f32, const void* Bw, void* C, int c_f32, int M, int N, int K,
                int64_t lda, int64_t ldb, int64_t ldc, const float* bias_n, const float* residual, float alpha,
                void* stream);
/* the same with the residual stored in the compute dtype (f16 / bf16) instead of fp32: the form the engine uses for
 * the residual stream between blocks in f16 mode */
int t2p_op_gemm_r16(int dtype, const void* A, int a_f32, const void* Bw, void* C, int c_f32, int M, int N, int K, int64_t lda,
                    int64_t ldb, int64_t ldc, const float* bias_n, const void* residual16, float alpha, void* stream);
/* the feed-forward's first product with the GEGLU gate in the epilogue: A [M][K] and Bw [N][K] in the 16-bit compute dtype, the rows
 * of Bw (and bias_n [N], optional) interleaved (value_j, gate_j); C [M][ldc >= N / 2] (compute dtype) = value * gelu_erf(gate).
 * T2P_ERR_INVALID when the product does not take the fused epilogue */
int t2p_op_gemm_geglu(int dtype, const void* A, const void* Bw, void* C, int M, int N, int K, int64_t ldc, const float* bias_n, void* stream);
/* x: NHWC in the given layout; w: [Cout][3][3][Cin] compute dtype; out fp32 NHWC */
int t2p_op_conv3x3(int dtype, const void* x, int a_f32, const void* w, const float* bias, float* out, int batch,
                   int H, int W, int Cin, int Cout, int upsample, void* stream);
/* second convolution of a residual block with its 1x1 shortcut in the same K loop (layers.py:322-327, h + Conv_2(x)):
 * out = alpha * (conv3x3(a) + [x0 | x1] Wx^T + bias); a, x0, x1: NHWC compute dtype (x1 may be NULL with CX1 = 0: the
 * second source of a concatenated block input); w: [Cout][9 * C + CX0 + CX1], the 3x3 taps first; out fp32 or compute
 * dtype.  16-bit modes on the LDS-DMA kernels only (C, CX0, CX1 multiples of 64): anything else is refused */
int t2p_op_conv3x3_shortcut(int dtype, const void* a, const void* w, const float* bias, const void* x0, int CX0,
                            const void* x1, int CX1, float alpha, void* out, int c_f32, int batch, int H, int W, int C,
                            int Cout, void* stream);
/* a 3x3 convolution FOLLOWED by a GroupNorm (+SiLU) of its output, as inside ResnetBlockBigGANpp.forward (layers.py:304-321:
 * h = Conv_0(...) + Dense_0(temb); h = act(GroupNorm_1(h)), and the block output -> the next block's GroupNorm_0): low-resolution
 * convolutions run with the K loop split over workgroups, and the pass that sums the partial tiles applies the norm too.
 * a [batch][H][W][C] and w [Cout][9 C] in the 16-bit compute dtype; bias [Cout], bias_bn [batch][Cout] (time-embedding bias) and
 * residual [batch][H][W][Cout] (compute dtype) optional; out (fp32 or compute dtype, may be null) = alpha (conv + biases + residual);
 * normed (compute dtype) = act(GroupNorm(out)); col_stats optional (per-64-row column sums of out, H W % 64 == 0).
 * T2P_ERR_INVALID when the launch would not take that plan (no workspace: t2p_debug_set(10, MiB); K loop too short; H W > 256) */
int t2p_op_conv3x3_groupnorm(int dtype, const void* a, const void* w, const float* bias, const float* bias_bn, const void* residual,
                             float alpha, int upsample, int groups, const float* gamma, const float* beta, float eps, int silu,
                             void* out, int out_f32, void* normed, float* col_stats, int batch, int H, int W, int C, int Cout, void* stream);
/* a 3x3 convolution of an 8x8 or 4x4 map with everything ResnetBlockBigGANpp.forward (layers.py:303-327) does around it, in ONE
 * launch with no second pass: a workgroup owns whole samples x whole GroupNorm groups (64 rows x 16 channels), so the norm that
 * follows is applied on the spot.  a [batch][H][W][C], w [Cout][ldw] (K index = tap C + c, then CX0 + CX1 shortcut columns read
 * at the output pixel from x0 | x1), residual [batch][H][W][Cout]: all in the 16-bit compute dtype; bias [Cout], bias_bn
 * [batch][Cout] fp32.  out (optional, fp32 or 16-bit) = alpha (conv + shortcut + biases + residual); col_stats (optional, 8x8
 * maps) its per-64-row column sums; normed (optional, 16-bit) = act(GroupNorm(out)) with `groups` groups of 8 or 16 channels.
 * H = W in {4, 8}, batch H W % 64 == 0, C % 32 == 0, Cout % 16 == 0. */
int t2p_op_small_conv_groupnorm(int dtype, const void* a, const void* w, int64_t ldw, const void* x0, int CX0, const void* x1, int CX1,
                                const float* bias, const float* bias_bn, const void* residual, float alpha, void* out, int out_f32,
                                float* col_stats, void* normed, int groups, const float* gamma, const float* beta, float eps, int silu,
                                int batch, int H, int W, int C, int Cout, void* stream);
/* row-wise chains of a SpatialTransformer block as ONE launch over 32-row blocks (model/attention.py:250-256 GroupNorm + proj_in,
 * :208-215 LayerNorm + residual adds, :170-193 to_q / to_k / to_v / to_out):
 *   t = a W_in^T + b_in (+ residual);  out2 = LayerNorm(t) W_2^T        (t [batch n][C], out2 [batch n][n2], 16-bit)
 * with a = GroupNorm(x) (statistics from col_stats, the per-64-row column sums of x, [batch n / 64][C][2]) or a = x (col_stats
 * NULL).  Entry of the block: W_in = proj_in, W_2 = to_q | to_k | to_v stacked (n2 = 3 C).  After the self-attention: x = its
 * output, W_in = to_out, residual = t (may alias the output t), W_2 = the cross-attention's to_q (n2 = C).  After the
 * cross-attention: the same with W_2 = ff.net.0 (n2 = 8 C, rows interleaved (value_j, gate_j), bias b_2) and geglu = 1:
 * out2 [batch n][4 C] = value * gelu_erf(gate) (model/attention.py:37-64).  With w_3 [C][5 C] (ff.net.2 and proj_out as one
 * matrix over [out2 | t], :213-215, 259-263), b_3 and res3 (the block input) a third product follows in the same launch:
 * y [batch n][C] = [out2 | t] W_3^T + b_3 + res3, y_stats its per-64-row column sums (out2 then stays on chip: out2 may be NULL).
 * x, w_in [C][C], w_2 [n2][C], residual in the 16-bit compute dtype.  C = 256, or C = 512 without geglu / w_3; n % 32 == 0
 * (n % 64 == 0 with col_stats), batch n <= 8192; anything else is refused */
int t2p_op_st_entry(int dtype, const void* x, const float* col_stats, int groups, const float* gn_gamma, const float* gn_beta,
                    float gn_eps, const void* w_in, const float* b_in, const void* residual, const float* ln_gamma,
                    const float* ln_beta, float ln_eps, const void* w_2, int n2, const float* b_2, int geglu, void* t, void* out2,
                    const void* w_3, const float* b_3, const void* res3, void* y, float* y_stats, int batch, int n, int C,
                    void* stream);
/* the projections of an AttnBlockpp (layers.py:160-167) in ONE launch over 32-row blocks at C = 256: h = GroupNorm(x) (statistics from
 * col_stats as in t2p_op_st_entry, or x already normalised), qk [batch n][2 C] = h [W_0 | W_1]^T + b (NIN_0 | NIN_1), and
 * vt [batch][C][npad] = (h W_v^T)^T: the value projection written transposed (the engine passes NIN_2 . NIN_3 as W_v).
 * x, w_qk [2 C][C], w_v [C][C], qk, vt in the 16-bit compute dtype.  n % 32 == 0, batch n <= 8192, npad >= n, npad % 4 == 0.
 * With k_fm (npad == n): the k half goes to k_fm and vt is written in the fragment-major order of t2p_op_attention_wide_fm instead */
int t2p_op_attn_proj(int dtype, const void* x, const float* col_stats, int groups, const float* gn_gamma, const float* gn_beta,
                     float gn_eps, const void* w_qk, const float* b_qk, const void* w_v, void* qk, void* vt, void* k_fm,
                     int64_t npad, int batch, int n, int C, void* stream);
/* the network's input convolution (pre_conv, ncsnpp.py:230: 3x3, C = 5 or 8 input channels -> nf) straight from the NCHW fp32
 * sample, in fp32 arithmetic: x [batch][C][H][W] fp32; w_tcn [3*3][C][nf] fp32 (tap-major); out NHWC [batch][H][W][nf] in
 * out_dtype.  col_stats (optional; W % 64 == 0, nf | 256): [batch H W / 64][nf][2] fp32 = (sum, sum of squares) of the fp32
 * results per 64-pixel chunk and channel -- what the first GroupNorm needs, so that it does not re-read the tensor.
 * 16-bit out_dtype with W % 64 == 0, an even H and nf in {64, 128, 256}: the layer runs on the 16-bit matrix pipe with every fp32
 * operand split into two f16 terms (fp32-class accuracy, ~2^-22; needs |x| < 65504 -- the engine takes this form for
 * sigma_max <= 4096); the call then returns after the stream has drained (it prepares the split weights in a temporary) */
int t2p_op_input_conv(const float* x, const float* w_tcn, const float* bias, void* out, int out_dtype, int batch, int C,
                      int H, int W, int nf, float* col_stats, void* stream);
int t2p_op_groupnorm(const float* x0, const float* x1, int C0, int C1, int batch, int H, int W, int groups,
                     const float* gamma, const float* beta, float eps, int silu, int down, void* out, int dtype,
                     void* stream);
int t2p_op_layernorm(const float* x, const float* gamma, const float* beta, void* out, int dtype, int64_t rows,
                     int C, float eps, void* stream);
/* the same on rows stored in the compute dtype (f16 / bf16), output in that dtype: the form the engine uses inside the
 * transformer blocks in 16-bit modes (attention.py:203-205) */
int t2p_op_layernorm16(const void* x16, const float* gamma, const float* beta, void* out16, int dtype, int64_t rows, int C,
                       float eps, void* stream);
int t2p_op_softmax(const float* S, int64_t lds, void* P, int64_t ldp, int dtype, int64_t rows, int n, float scale,
                   void* stream);
int t2p_op_geglu(const float* u, void* out, int dtype, int64_t rows, int inner, void* stream);
/* q: [B][nq][ldq], k: [B][nk][ldk] (head h at column h*d), vt: [B][heads*d][ldvt]; out [B][nq][heads*d].
 * Operands in compute dtype; scores/softmax in fp32.  workspace sizes via t2p_op_attention_ws. */
int64_t t2p_op_attention_ws(int dtype, int batch, int heads, int nq, int nk);
int t2p_op_attention(int dtype, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt,
                     int64_t ldvt, void* out, int batch, int heads, int nq, int nk, int d, float scale,
                     void* workspace, void* stream);
/* AttnBlockpp.forward after its projections (layers.py:168-176: w = softmax(q k^T / sqrt C) over ALL h w pixels, ONE head of
 * width d = C; h = w v; (x + NIN_3(h)) / sqrt 2) in one launch: q, k [batch][n][ld*] and vt = v^T [batch][d][ldvt] in the 16-bit
 * compute dtype -- the engine folds NIN_3 into the value projection (rows of w sum to 1), so what remains of the block's tail is
 * out[batch][n][d] = alpha (w v + bias[d] + residual[batch][n][d]), stored fp32 (out_f32) or in the compute dtype; col_stats
 * (optional, n % 64 == 0): [batch n / 64][d][2] column sums / sums of squares of out's fp32 values per 64 queries (the next
 * GroupNorm's input).  d = 256 / 512 / 1024, n <= 1024 (<= 512 at d = 1024), n % 8 == 0. */
int t2p_op_attention_wide(int dtype, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, void* out,
                          int out_f32, const float* bias, const void* residual, int residual_16bit, float alpha, float* col_stats,
                          int batch, int n, int d, float scale, void* stream);
/* the same with k and vt FRAGMENT-MAJOR ([batch][n d] each: element (r, c) -- r = key, c = channel for k; r = channel, c = key for
 * vt -- at ((r / 32) (cols / 32) + c / 32) 1024 + ((c / 8) % 2) 512 + ((c / 16) % 2) 256 + (r % 32) 8 + c % 8): the kernel's fragment
 * loads are then 1 KiB contiguous.  d = 512 with 512 < n <= 1024, or d = 256 with n <= 256; n % 32 == 0.  Bit-identical to
 * t2p_op_attention_wide. */
int t2p_op_attention_wide_fm(int dtype, const void* q, int64_t ldq, const void* k_fm, const void* vt_fm, void* out, int out_f32,
                             const float* bias, const void* residual, int residual_16bit, float alpha, float* col_stats, int batch,
                             int n, int d, float scale, void* stream);
/* C = A Bw^T (16-bit, [M][N] row-major; batch > 1: A [M][K] shared, Bw [batch][N][K], C [batch][M][N]) with the columns from
 * frag_col0 on written fragment-major into c_frag instead (layout above; per sample of rows_per_batch rows, or per batch entry):
 * what the engine asks of the q | k projection and of the transposed value projection of an AttnBlockpp (layers.py:163-167).
 * Refused unless the product runs on the 256 x 256 register-epilogue kernel with whole 32 x 32 fragments */
int t2p_op_gemm_frag_major(int dtype, const void* A, const void* Bw, void* C, void* c_frag, int M, int N, int K, int frag_col0,
                           int rows_per_batch, int batch, void* stream);
/* self-attention on the output of ONE stacked projection (CrossAttention.forward with context = x, model/attention.py:
 * 170-191): qkv [batch][n][ld] holds q | k | v in three column blocks of heads*d (head h at column h*d of its block);
 * out [batch][n][heads*d].  V is read row-major -- the fused kernel transposes it on the way out of LDS -- so no
 * separate V^T projection is needed.  16-bit dtypes, d in {32, 64, 128} only (anything else is refused) */
int t2p_op_attention_qkv(int dtype, const void* qkv, int64_t ld, void* out, int batch, int heads, int n, int d,
                         float scale, void* stream);
int t2p_op_langevin(const float* x, const float* grad, const float* noise, const uint8_t* mask,
                    const float* x_initial, float* x_out, float* x_mean_out, int batch, int64_t per_sample,
                    float snr, float alpha, float* sums_out /* device float[2], may be NULL */, void* stream);
/* split form: norms -> (optional all-reduce of sums over ranks by the caller) -> update.
 * workspace: device float[batch * 128]; sums: device float[2] = {sum_b ||grad_b||, sum_b ||noise_b||} */
int t2p_op_langevin_norms(const float* grad, const float* noise, int batch, int64_t per_sample, float* workspace,
                          float* sums, void* stream);
int t2p_op_langevin_update(const float* x, const float* grad, const float* noise, const uint8_t* mask,
                           const float* x_initial, float* x_out, float* x_mean_out, int64_t n, const float* sums,
                           float batch_total, float snr, float alpha, void* stream);
int t2p_op_predictor(const float* x, const float* score, const float* noise, const uint8_t* mask,
                     const float* x_initial, float* x_out, float* x_mean_out, int64_t n, float G,
                     int probability_flow, void* stream);
/* The three kernels of a guided PC step as operators, every scalar by value.  The score is s = scale (w o_c + w1 o_u), each product
 * and sum of the guidance sum rounded to float32 in this order (w1 = (float)(1 - w) as the reference rounds it; scale: 1 for VE,
 * -1 / std for VP); o_u NULL: s = scale o_c.
 *   norms:     sums = {sum_b ||s_b||, sum_b ||noise_b||}, workspace as t2p_op_langevin_norms
 *   langevin:  t2p_op_langevin_update on s;   predictor: x_mean = x_coef x + G^2 s (halved under probability_flow), as t2p_op_predictor
 * With o_u NULL and scale == 1 (and x_coef == 1) the two updates equal t2p_op_langevin_update / t2p_op_predictor bit for bit.
 * x_out may alias x; x_out2 (optional) receives a second copy of the new state; x_mean_out is optional.  n % 4 == 0 with every
 * pointer 16-byte aligned (the mask 4-byte) takes 16-byte accesses, anything else goes element by element. */
int t2p_op_guided_langevin_norms(const float* o_c, const float* o_u, const float* noise, int batch, int64_t per_sample, float w, float w1,
                                 float scale, float* workspace, float* sums, void* stream);
int t2p_op_guided_langevin_update(const float* x, const float* o_c, const float* o_u, const float* noise, const uint8_t* mask,
                                  const float* x_initial, float* x_out, float* x_out2, float* x_mean_out, int64_t n, float w, float w1,
                                  float scale, const float* sums, float batch_total, float snr, float alpha, void* stream);
int t2p_op_guided_predictor(const float* x, const float* o_c, const float* o_u, const float* noise, const uint8_t* mask,
                            const float* x_initial, float* x_out, float* x_out2, float* x_mean_out, int64_t n, float w, float w1,
                            float scale, float G, float x_coef, int probability_flow, void* stream);
/* The two update kernels of a PC step WITH the replacement of t2p_sampler_set_inpaint, the kernels the loop runs: arguments as
 * t2p_op_guided_langevin_update / t2p_op_guided_predictor (o_u NULL: the plain forms), then the replacement.  (a, s) are the
 * values mean_coef / std, or, with device tables of n_table floats, row `step` of them.  noise: device z, or NULL = drawn in the
 * kernel as t2p_op_philox_normal(seed, stream_id) draws with `step` in the step word.  The 16-byte path additionally needs data and
 * noise 16-byte and known 4-byte aligned. */
typedef struct t2p_inpaint_replace {
  const uint8_t* known;       /* device uint8, 1 = known */
  const float* data;          /* device fp32 */
  const float* noise;         /* device fp32 or NULL */
  const float* mean_table;    /* device fp32[n_table] or NULL (with std_table) */
  const float* std_table;
  int32_t n_table;
  int32_t step;
  float mean_coef, std;
  uint64_t seed, stream_id;
} t2p_inpaint_replace;
int t2p_op_inpaint_langevin_update(const float* x, const float* o_c, const float* o_u, const float* noise, const uint8_t* mask,
                                   const float* x_initial, float* x_out, float* x_out2, float* x_mean_out, int64_t n, float w, float w1,
                                   float scale, const float* sums, float batch_total, float snr, float alpha,
                                   const t2p_inpaint_replace* replace, void* stream);
int t2p_op_inpaint_predictor(const float* x, const float* o_c, const float* o_u, const float* noise, const uint8_t* mask,
                             const float* x_initial, float* x_out, float* x_out2, float* x_mean_out, int64_t n, float w, float w1,
                             float scale, float G, float x_coef, int probability_flow, const t2p_inpaint_replace* replace, void* stream);
int t2p_op_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);
int t2p_op_convert(const float* in, void* out, int dtype, int64_t n, void* stream);
/* One weight packing of t2p_engine_load_flat on caller-supplied device buffers: fp32 sources -> dst in `dtype`.  kind / dims (a pitch or
 * cin_pad of 0 = dense):
 *   0 copy     src0|src1|src2 concatenated            n0, n1, n2
 *   1 rows     (rows, rowlen) -> dst[r ld + j]        rows, rowlen, ld
 *   2 conv3    (N, Ci, 3, 3) -> [N][tap][cin_pad]     N, Ci, cin_pad, ld          channels past Ci zero
 *   3 conv3_t  (N, C, 3, 3) -> [tap][C][N]            N, C
 *   4 nin      one / two (K, N) -> [nsrc N][K]        K, N, nsrc
 *   5 geglu    (2 inner, rowlen), rows interleaved    inner, rowlen               (value_j, gate_j)
 *   6 up4      (co, ci, 3, 3) -> [4][co][4][ci]       co, ci                      taps summed in fp32 in (kh, kw) order
 *   7 add      src0 + src1                            n
 *   8 product  src0 (M, K) src1 (K, N) [+ src2 (N)]   M, K, N, transposed, ld     fp32, ascending k, product and add each rounded
 *   9 dot64    src2[n] + sum_j src0[n][j] src1[j]     N, K                        accumulated in double, rounded once */
int t2p_op_weight_pack(int kind, const float* src0, const float* src1, const float* src2, void* dst, const int64_t* dims, int ndims, int dtype,
                       void* stream);
/* ---- either side of the sampler ----
 * 6D decode of finished samples, sampling_rosetta.py:69-96: x = (batch, channels, L, L) fp32 with the padding mask in
 * the last channel.  lengths[b] = sqrt(#(round(mask) == 1)) or -1 when that count is not a perfect square (the
 * reference raises ValueError); clipped / absval = (batch, 4, L*L) fp32: per channel (dist, omega, theta, phi) the
 * first lengths[b]^2 entries are clip(x[c][mask == 1], -1, 1) in row-major order (= .reshape(L, L)) and its inverse
 * scaling (dist+1)*10, omega*pi, theta*pi, (phi+1)*pi/2. */
int t2p_op_decode_6d(const float* x, int batch, int channels, int L, float* clipped, float* absval, int32_t* lengths, void* stream);
/* 6D encode of backbones, the featuriser behind utils.py:108-137: dataset.py:396-450 (get_coords6d: virtual Cb, Cb-Cb distance
 * within 20 A, omega / theta dihedrals, phi angle, normalised to [-1, 1]), :200-239 (residue and pair masks, padding channel, every
 * channel times mask_pair) and :114-168 (get_coarse_constraints: helix, beta and block-adjacency channels), padded as PaddingCollate
 * does (:452-506).  xyz = (batch, L, 3, 3) fp32 device, N / CA / C per residue; nres = (batch) int32 device; atom_ok = (batch, L, 3)
 * uint8 device or NULL (every atom present; a missing atom counts as (0, 0, 0) whatever xyz holds).  channels = 5, or 8 with the
 * three secondary-structure channels at 4:7.  host_blocks = n_blocks int32 quadruples (sample, start, last, kind) on the HOST,
 * kind 0 helix / 1 beta, per sample the helices first, then the strands, each in chain order (the order of the reference's
 * "start:last" string); the range is the reference's half-open [start:last], `last` being the block's last residue.  Only with
 * channels = 8; without blocks channels 4:7 are zero.  Outputs: coords_6d = (batch, channels, L, L) fp32, mask_pair =
 * (batch, L, L) uint8, every element written.  Refused before anything is launched (status and message, outputs untouched):
 * nres[b] outside [1, L], a block outside [0, nres) of its sample, start > last, a sample index outside the batch, a kind other
 * than 0 / 1, blocks with channels = 5, any other channel count.  nres is read back on the host: the call synchronises the stream. */
int t2p_op_encode_6d(const float* xyz, const int32_t* nres, const uint8_t* atom_ok, int batch, int channels, int L,
                     const int32_t* host_blocks, int n_blocks, float* coords_6d, uint8_t* mask_pair, void* stream);
/* Secondary structure from CA traces, the annotation the reference asks biotite for (struc.annotate_sse, dataset.py:121-123): P-SEA
 * (Labesse et al. 1997) with its published thresholds as biotite applies them, restated in DESIGN.md 8i, which is normative -- no
 * biotite release is the yardstick.  One workgroup per chain, in double from the fp32 coordinates.
 *   xyz = (batch, L, atoms, 3) fp32 on the device; atoms = 3: the N / CA / C layout of t2p_op_fold_6d and t2p_op_encode_6d, of which
 *   atom 1 is read; atoms = 1: a bare CA trace (the convention of t2p_op_tm_align).  len = (batch) int32; nothing past len[b] is read.
 *   atom_ok = (batch, L, atoms) uint8 or NULL (every atom present).  A residue whose CA is absent has no CA; a residue whose CA
 *   coordinate is not finite or exceeds 1e6 in magnitude is treated as absent and status[b] = 1.
 *   target = (batch, L) uint8 letters or NULL.
 * Outputs, device, every element written:
 *   letters = (batch, L) uint8: ASCII 'a' (helix) / 'b' (strand) / 'c' inside the length, 0 past it.  A residue without a CA is 'c'
 *   (the reference drops such a chain, dataset.py:124);
 *   counts = (batch, 12) int32: residues a, b, c; runs of a of at least 4 and runs of b of at least 4 (the blocks of
 *   encode.sse_blocks); residues with target a and, of those, the ones labelled a; the same two for b (all four 0 without a target);
 *   residues without a CA; 0; 0;
 *   status[b] = 0, 1 as above, or -1 when len[b] lies outside [1, L]: that chain's letters and counts are then zero.
 * Refused before launch (status and message): L outside [1, 512] (the fold's limit), atoms other than 1 or 3, batch <= 0, a null xyz,
 * len, letters, counts or status.  No workspace; everything is enqueued on `stream`; nothing is read back; only integers are counted,
 * so two calls give the same bits. */
int t2p_op_annotate_sse(const float* xyz, const int32_t* len, const uint8_t* atom_ok, int batch, int L, int atoms, const uint8_t* target,
                        uint8_t* letters, int32_t* counts, int32_t* status, void* stream);
/* Backbones from decoded maps, in place of the reference's PyRosetta stage (sampling_rosetta.py:98-160) -- restraint-free: known pairs
 * (dist < known_below, upper triangle), geodesic completion, classical MDS, stress_steps refinement steps on the Cb trace, N / CA / C
 * from phi, theta and the featuriser's virtual-Cb identity, the mirror image told apart by chain closure.  absval =
 * (batch, 4, L*L) fp32 and lengths = (batch) int32, both on the device, as t2p_op_decode_6d writes them; L <= 512.  Outputs, device:
 * xyz = (batch, L, 3, 3) fp32, zero past lengths[b]; status[b] = 0 ok, 1 when the known-pair graph is disconnected or a residue had
 * fewer than 3 neighbours (dist <= 12) or a singular system -- such a residue takes the offsets of the nearest framed residue and
 * placed[b * L + i] = 1 -- and -1 for an improper mask (coordinates zero); diag = (batch, 16) double: hand kept (0 = the embedding whose
 * axes rise along the chain, 1 = its mirror), closure error mean | |C_i - N_i+1| - 1.329 | of hand 0 and of hand 1, stress rms over the
 * known pairs, the four restraint scores (dist, omega, theta, phi) and their four counts as t2p_op_restraint_score gives them,
 * unreachable pairs, the three leading eigenvalues.  Every output is finite.  workspace = t2p_op_fold_ws(batch, L) bytes on the device
 * (-1: L out of range).  Everything is enqueued on `stream`; nothing is read back. */
int64_t t2p_op_fold_ws(int batch, int L);
int t2p_op_fold_6d(const float* absval, const int32_t* lengths, int batch, int L, float known_below, int stress_steps, float dist_std,
                   float angle_std, float* xyz, int32_t* status, uint8_t* placed, double* diag, void* workspace, int64_t workspace_bytes,
                   void* stream);
/* TM-align on the device, what the reference does with its backbones next: tm/TMalign.py:36-61 (tm_score, max_min_avg_tm_score),
 * :63-160 (train_gen_tm_compare), utils.py:150-158 (run_tmalign, one subprocess of tm/TMalign.cpp per pair) and play.py:49-61.  The
 * default path of TMalign.cpp for n_pairs pairs of CA traces, one workgroup per pair, in double.
 *   xyz_a = (n_a, La, atoms_a, 3), xyz_b = (n_b, Lb, atoms_b, 3) fp32 on the device; atoms = 3: the N / CA / C layout of t2p_op_fold_6d,
 *   of which atom 1 is read; atoms = 1: a bare CA trace.  len_a (n_a), len_b (n_b) int32; nothing past len[c] is read.
 *   pairs = (n_pairs, 2) int32 on the device (index into a, index into b), or NULL for all n_a x n_b pairs in row-major order.
 * Chain a is TM-align's Chain_1, the one superimposed; chain b is Chain_2.  Outputs, device:
 *   out8[p] = TM-score normalised by len_a, by len_b, RMSD of the pairs within score_d8 (rmsd0), their count n_ali8, d0 for len_a, d0
 *   for len_b, the search stage's TMmax, the index 0..4 of the seed that produced the final alignment (get_initial, get_initial_ss,
 *   get_initial5, get_initial_ssplus, get_initial_fgt);
 *   b2a = (n_pairs, Lb) or NULL: for each residue of b the aligned residue of a among the pairs within score_d8 (the alignment
 *   TM-align prints), else -1; -1 past len_b;
 *   rot12 = (n_pairs, 12) or NULL: t[3] then u[3][3] of the superposition of a onto b that belongs to the score normalised by len_b
 *   (what TM-align's -m prints);
 *   status[p] = 0, or 1 when a chain of the pair is shorter than 5 or longer than TM_MAX_L = 256 residues (or than La / Lb): out8 and
 *   rot12 are then zero, the map -1, and the other pairs are unaffected.  TM-align's own floor is 3 residues, but its seeds degenerate
 *   below min_ali = 5, and no chain here is shorter than data.min_res_num = 40.
 *   status[p] is also 1, with the same zero outputs, when a coordinate of either chain inside its length is not finite or exceeds
 *   1e6 in magnitude: every distance would be NaN and TM-align's own threshold-relaxation loops would never end (the reference's
 *   process hangs on such a file); the kernel checks both traces as it loads them and additionally caps those loops.
 * workspace = t2p_op_tm_align_ws(n_pairs, La, Lb) bytes on the device: a fixed 256 bytes whatever the arguments, or -1 when La or Lb
 * is above TM_MAX_L or any of the three is not positive.  Its first int32 is a flag the call zeroes and the kernel sets when a pair
 * index lies outside its set (that pair gets status 1); the caller reads it after the call, as with t2p_op_embedding_gather's
 * bad_flag.  Refused before launch: a workspace too small, atoms other than 1 or 3, non-positive counts.  Everything is enqueued on
 * `stream`; nothing is read back. */
int64_t t2p_op_tm_align_ws(int n_pairs, int La, int Lb);
int t2p_op_tm_align(const float* xyz_a, const int32_t* len_a, int n_a, int La, int atoms_a, const float* xyz_b, const int32_t* len_b, int n_b,
                    int Lb, int atoms_b, const int32_t* pairs, int n_pairs, double* out8, int32_t* b2a, double* rot12, int32_t* status,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* The reference's restraint set (load_constraints, rosetta_min/utils.py:119-206) scored on given backbones xyz = (batch, L, 3, 3) with
 * the harmonic forms Rosetta applies, in double, Cb being the virtual Cb: out8 = (batch, 8) double = sums over dist (i < j,
 * 0 < d <= 12, ((|Cb_i - Cb_j| - d) / dist_std)^2), omega (i < j, omega != 0, d <= 12, circular), theta (ordered pairs a != b with
 * d[a][b] <= 12, circular) and phi (the same pairs, harmonic), angle_std in degrees, then the four counts.  Workspace as above. */
int t2p_op_restraint_score(const float* xyz, const float* absval, const int32_t* lengths, int batch, int L, float dist_std, float angle_std,
                           double* out8, void* workspace, int64_t workspace_bytes, void* stream);
/* Refinement of backbones against the same restraint set, the stage the reference runs between the maps and TM-align
 * (rosetta_min/run.py) -- not Rosetta: a Cartesian L-BFGS on N / CA / C, in double, one persistent workgroup per chain, nothing read back.
 * The energy: the four restraint terms of t2p_op_restraint_score with the same sets and forms, less the theta restraints whose target phi
 * lies within arm_min degrees of 0 or 180 and the omega restraints for which phi_ij or phi_ji does, counted for sep_lo <= |i - j| <
 * sep_hi; plus bonds (N-CA 1.458, CA-C 1.525, C-N 1.329, sigma 0.02 A), angles (N-CA-C 111.0, CA-C-N 116.2, C-N-CA 121.7, sigma 3
 * degrees), peptide planarity (dihedral CA C N CA about 180, sigma 6 degrees), each ((x - x0) / sigma)^2, and the repulsion
 * max(0, 3.8 - |CA_i - CA_j|)^2 over j - i >= 2.  E = w_dist dist + w_ang (omega + theta + phi) + bond + angle + pept + w_rep rep.
 *   xyz_in = (batch, L, 3, 3) fp32, absval = (batch, 4, L*L) fp32 and lengths = (batch) int32 as t2p_op_fold_6d takes and writes them;
 *   L <= 256.  schedule = n_stages (1..8) x 6 doubles on the HOST: sep_lo, sep_hi, w_dist, w_ang, w_rep, max_iter.  Per stage: L-BFGS
 *   (8 pairs), Armijo backtracking (c1 1e-4, halving, 20 trials), steepest descent on a non-descent direction or after a failed line
 *   search, stop at max|g| < 1e-3.  dist_std in A, angle_std and arm_min in degrees.
 * Outputs, device: xyz_out = (batch, L, 3, 3) fp32, zero past lengths[b]; status[b] = 0 ok, 1 a stage ended on a failed line search
 * (the coordinates are the best accepted), 2 a coordinate of the start is not finite (zeros), -1 lengths[b] < 2 or > L (zeros);
 * diag = (batch, 16) double: E at the start under the last stage's weights, E at the end, the eight unweighted terms at the end (dist,
 * omega, theta, phi, bond, angle, pept, rep), line searches run, energy evaluations, final max|g|, final mean closure error
 * | |C_i - N_i+1| - 1.329 |, stages completed, 0.  Every output is finite.  workspace = t2p_op_refine_ws(batch, L) bytes on the device
 * (-1: L above 256 or an argument not positive).  Two calls give the same bits, whatever batch or padding a chain sits in. */
int64_t t2p_op_refine_ws(int batch, int L);
int t2p_op_refine_backbone(const float* xyz_in, const float* absval, const int32_t* lengths, int batch, int L, const double* schedule,
                           int n_stages, float dist_std, float angle_std, float arm_min, float* xyz_out, int32_t* status, double* diag,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* One evaluation of that energy, by the device functions the minimiser calls: stage = 6 doubles on the host (max_iter ignored);
 * out9 = (batch, 9) double = the eight unweighted terms and the weighted total, grad = (batch, L, 3, 3) double = the gradient of the
 * total, zero past lengths[b]; all zero for a chain t2p_op_refine_backbone would give status 2 or -1.  Workspace as above. */
int t2p_op_restraint_energy(const float* xyz, const float* absval, const int32_t* lengths, int batch, int L, const double* stage,
                            float dist_std, float angle_std, float arm_min, double* out9, double* grad, void* workspace,
                            int64_t workspace_bytes, void* stream);
/* The reference's "diversify backbone" move (rosetta_min/run.py:104-109) on N / CA / C chains held in Cartesian coordinates (DESIGN.md
 * 8j).  Atoms a_0 .. a_3n-1 run N, CA, C per residue, read as double from fp32.  For k >= 3: b_k = |a_k - a_k-1|, theta_k the angle at
 * a_k-1, tau_k = dihedral(a_k-3, a_k-2, a_k-1, a_k).  tau_3i+2 (phi_i) takes + dphi_i for i >= 1, tau_3i+3 (psi_i) + dpsi_i for
 * i <= n - 2; omega, bond lengths and bond angles stay as measured.  Atoms 0..2 are copied, every later atom is rebuilt from the three
 * rebuilt atoms before it (NeRF); where that frame is undefined (three collinear atoms) the atom is placed with tau unchanged in the
 * fallback frame DESIGN.md 8j states.  Draws: Philox4x32-10, key = seed, training layout, counter {residue i, chain_ids[b], stream lo,
 * stream hi}; dphi_i = amp_deg (2 u(word 0) - 1), dpsi_i = amp_deg (2 u(word 1) - 1) degrees.  chain_ids = (batch) int32 on the
 * device, or null for 0 .. batch - 1: a chain's move does not depend on its batch position or padding.
 *   xyz_in = (batch, L, 3, 3) fp32, lengths = (batch) int32, L <= 256, replicas in 1..16.  xyz_out = (batch, replicas, L, 3, 3) fp32,
 *   zero past lengths[b]: candidate k draws under stream + k; with keep_first != 0 candidate 0 is a bit-exact copy of the input.
 *   status = (batch, replicas) int32: 0 ok, 2 a coordinate not finite (zeros), -1 lengths[b] < 2 or > L (zeros).  Always finite. */
int t2p_op_perturb_torsions(const float* xyz_in, const int32_t* lengths, const int32_t* chain_ids, int batch, int L, int replicas,
                            float amp_deg, uint64_t seed, uint64_t stream, int keep_first, float* xyz_out, int32_t* status,
                            void* stream_handle);
/* Refinement in rounds: the loop of rosetta_min/run.py:88-151 on the device.  Per chain the incumbent starts as xyz_in
 * with E_inc = +inf; round r perturbs it into `replicas` candidates (t2p_op_perturb_torsions, stream = stream_base + 16 r, keep_first in
 * round 0 only), minimises each as t2p_op_refine_backbone does under schedules[r] (batch x replicas workgroups in one launch), scores
 * each with the weighted total of t2p_op_restraint_energy under select_stage (E_sel), and the lowest E_sel among the candidates of
 * status 0 or 1 (ties: the lowest index) replaces the incumbent when it is below E_inc.  Four launches per round on `stream`, nothing
 * read back.  schedules = rounds x n_stages x 6 doubles and select_stage = 6 doubles on the HOST; rounds in 1..8, replicas in 1..16,
 * batch x replicas <= 65535.
 *   Outputs, device: xyz_out (batch, L, 3, 3) fp32, status (batch) and diag (batch, 16) = the kept candidate's, as
 *   t2p_op_refine_backbone writes them -- when no candidate was ever valid, the status t2p_op_refine_backbone gives xyz_in, with zeros;
 *   trace = (batch, rounds, replicas, 4) double: E_sel, status, energy evaluations, 1 where that candidate became the incumbent.
 *   workspace = t2p_op_refine_rounds_ws(batch, L, rounds, replicas) bytes (it does not grow with rounds; -1: L above 256, rounds or
 *   replicas out of range, or an argument not positive).  rounds = replicas = 1 gives t2p_op_refine_backbone's bits. */
int64_t t2p_op_refine_rounds_ws(int batch, int L, int rounds, int replicas);
int t2p_op_refine_rounds(const float* xyz_in, const float* absval, const int32_t* lengths, const int32_t* chain_ids, int batch, int L,
                         const double* schedules, int rounds, int n_stages, int replicas, const double* select_stage, float amp_deg,
                         uint64_t seed, uint64_t stream_base, float dist_std, float angle_std, float arm_min, float* xyz_out,
                         int32_t* status, double* diag, double* trace, void* workspace, int64_t workspace_bytes, void* stream);
/* text context = embed_tokens(ids), sampling_6d.py:134-137: out[(b,t)][:] = table[ids[(b,t)]][:] as fp32; the table
 * ([vocab][dim], fp32 / bf16 / f16 by table_dtype) stays resident.  *bad_flag (device int, zeroed by the caller) is
 * set to 1 when an id falls outside [0, vocab). */
int t2p_op_embedding_gather(const void* table, int table_dtype, const int32_t* ids, float* out, int64_t n_tokens, int dim, int vocab,
                            int32_t* bad_flag, void* stream);
/* x = where(mask, x, x_initial) (sampling.py:283,285,287) */
int t2p_op_apply_mask(float* x, const uint8_t* mask, const float* x_initial, int64_t n, void* stream);

/* ---- measurement hooks (bench.py): time every MFMA GEMM launch with HIP events on its stream ----
 * out9 = {LDS-DMA conv3x3: ms, flops, launches; other GEMMs: ...; conv3x3 on the register-staged kernel: ...} since t2p_profile_begin */
int t2p_profile_begin(void);
/* Plan switches for tests and A/B measurements: they select between kernel geometries / fusions that all
 * produce correct results (key 0 LDS-DMA GEMM on/off, 2 tile geometry, 3 split-K, 4..25 individual fusions and
 * kernel forms -- the full list is the key table next to t2p_debug_set, with every default and one line each in
 * text2protein_amd/csrc/plan.h and tools/README.md; key 48, read by t2p_train_create:
 * the 16-bit training step's fixed-order reductions, scaled backward seed and overflow guard on f32 products).  Key 1 is the
 * timing-only ablation mask of the LDS-DMA kernel: its bits 128 / 256 (DMA issue order) and 4096 (LDS-staged instead of
 * register epilogue), results unchanged, are always accepted, the bits that skip work and so produce
 * WRONG results exist only in a library built with -DT2P_ABLATION (python -m text2protein_amd.build --ablation)
 * and are refused (status 1) by the product build. */
int t2p_debug_set(int key, int value);
/* the current value of a plan switch (0 / 1 for the on / off switches, MiB for key 10); status 1 for an unknown key or a null pointer */
int t2p_debug_get(int key, int* value);
/* the short lowercase name of a plan switch (its member of t2p::Plan), or NULL for an unknown key */
const char* t2p_debug_key_name(int key);
/* launches of the row-resident K = 512 GEMM (plan switch 49) since the library was loaded: lets a test see which plan a launch took */
int64_t t2p_debug_rowres_launches(void);
/* not part of the stable ABI (a measurement aid of tools/bench_tmalign.py and tests/test_gpu_tmalign.py): out4 (host) = the wavefronts
 * and the dynamic LDS bytes of a t2p_op_tm_align workgroup at padded lengths La, Lb, then the kernel's registers per lane and scratch
 * bytes per lane as the loaded code object reports them */
int t2p_debug_tm_align_info(int La, int Lb, int32_t* out4);
/* 1 when the library was built with -DT2P_ABLATION (never the shipped one) */
int t2p_built_with_ablation(void);
int t2p_profile_end(double* out9);
/* after t2p_profile_end: the 3x3-convolution kernel instantiation with the largest total time in that region --
 * out4 = {ms (main kernel only), flops, launches, algorithmic bytes (inputs, weights, residual and output once each)},
 * name = the kernel name as rocprofv3 reports it (no argument list), so that bench.py's live average launch duration
 * can be checked against profiles/<round>_kernel_stats.csv and the PMC traffic against the algorithmic bytes */
int t2p_profile_dominant(double* out4, char* name, int name_len);
/* after t2p_profile_end: the fused-attention launches of that region (CrossAttention.forward, model/attention.py:181-191,
 * self and text cross-attention): out3 = {ms, flops (4 nq nk d per head), launches} */
int t2p_profile_attention(double* out3);
/* after t2p_profile_end: the GEMM / convolution launches of that region by operand shape, as CSV text
 * "kind,M,N,K,taps,batch,launches,ms,flops" (kind as in out9; K "a+b" = a channels per tap + b shortcut columns;
 * taps negative = gathered from the half-resolution map).  T2P_ERR_INVALID when the buffer is too small */
int t2p_profile_shapes(char* buf, int len);
/* after t2p_profile_end: the 3x3-convolution launches of that region on the LDS-DMA kernels by kernel instantiation and operand
 * shape, as text lines "kernel;M;N;K;launches" (the name as t2p_profile_dominant gives it; K = channels per tap): which tile geometry
 * every convolution of a pass ran, not only the dominant one.  T2P_ERR_INVALID when the buffer is too small */
int t2p_profile_conv_kernels(char* buf, int len);
/* per-block timing of the score network (UNetModel.forward, ncsnpp.py:220-263): HIP events on the launch stream at every block
 * boundary between _begin and _end; _end synchronises the device and writes CSV lines
 * "prefix,kind,map side,in channels,out channels,ms" in launch order (pre = embedding + input convolution, head = out.*) */
/* development: from now on every score evaluation also writes the output of block number `block_index` (launch order of
 * t2p_profile_layers_*, the pre / head entries not counted; -1 = off) to `dst` as fp32 NHWC [batch][H][W][C] (capacity in floats);
 * shape4 (optional) receives {C, H, W, stored-in-16-bit flag} of the LAST tap taken */
int t2p_debug_tap(int block_index, float* dst, int64_t capacity, int64_t* shape4);
int t2p_profile_layers_begin(void);
int t2p_profile_layers_end(char* buf, int len);

#ifdef __cplusplus
}
#endif
#endif /* T2P_H_ */
