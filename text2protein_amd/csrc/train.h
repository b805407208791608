// Training step of the score network: forward pass that keeps what the backward pass needs, backward pass,
// denoising score-matching loss, Adam / warm-up / clipping and the EMA update (reference score_sde_pytorch/losses.py:26-186,
// score_sde_pytorch/models/ema.py:32-49).  compute_dtype F32: exact-f32 products; F16 / BF16: 16-bit products with fp32 accumulation,
// everything the optimizer sees (parameters, gradients, moments, EMA, loss) fp32.  Every operator of the network (linear, conv3x3,
// group_norm, layer_norm, attention, add_scale) is one member that runs its forward and appends its backward to the tape; the
// dtypes differ inside tg (which strided GEMM), conv3x3 (which implicit GEMM) and in plumbing16_ (which form of the reductions, the
// scaled backward seed, the overflow guard).
#pragma once
#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "engine.h"
#include "train_kernels.h"

namespace t2p {

// plan switch 48 (g_plan.train_plumbing16): a trainer CREATED while it is set uses everything the 16-bit step uses except the products --
// the fixed-order reductions, the scaled backward seed (host power of two for VE, seed_scale on the device for VP / sub-VP) and the
// overflow guard -- with tg and conv3x3 on the f32 kernels.  Off by default; the product path never sets it

struct TParam {           // one learnable tensor: a slice of the flat buffers, in the reference's parameters() order
  std::string name;
  std::vector<int64_t> shape;
  long off = 0, n = 0;
};

struct TT {               // an NHWC activation [B][H W][C] fp32 of the training pass and its gradient (allocated on first use)
  float* p = nullptr;
  float* g = nullptr;
  int B = 0, H = 0, W = 0, C = 0;
  bool needs_grad = true;
  long rows() const { return (long)B * H * W; }
  long numel() const { return rows() * C; }
};

// ---- the 3x3 convolution of the training step ----------------------------------------------------------------------------------------------
// One statement of its products, run by Trainer::conv3x3 and by t2p_op_train_conv3x3 (include/t2p.h) alike: explicit buffers, and
// pass-local device memory through ConvScratch (the trainer: its pool; the operator entry: hipMalloc, freed after the call).
struct ConvScratch {
  std::function<void*(size_t)> get;     // bytes -> device block, nullptr when there is none
  std::function<void(void*)> put;       // stream-ordered: the next user of the block runs after the launches that used it
};
struct ConvW {            // one convolution's weights in the kernels' layouts (launch_conv_w_prep) and their 16-bit copies (or nullptr)
  int Co = 0, Ci = 0, Cip = 0, Cop = 0;
  const float* wf = nullptr; const float* wd = nullptr;
  const void* wf16 = nullptr; const void* wd16 = nullptr;
};
// one strided product: launch_tgemm (dt = DT_F32) or launch_tgemm16 with its workspace from sc
int train_tgemm(int dt, const TGemmArgs& a, const ConvScratch& sc, hipStream_t s);
// out [nz][N] += the column sums of the nz blocks of `rows` rows of dy; fixed_order: through a workspace from sc, else atomics
int train_colsum(const float* dy, int nz, long rows, int N, long ld, float* out, bool fixed_order, const ConvScratch& sc, hipStream_t s);
// one launch of the engine's implicit-GEMM 3x3 convolution (forward and data gradient): y [B][H W][ldc] = conv3x3(x) + bias
// (+ bias_bn[b][:]) (+ residual_inplace, which may be y), N columns written.  w16 == nullptr: the exact-f32 kernel on w; else the
// 16-bit kernels of dtype dt on w16 and on a 16-bit copy of x made here
int train_conv_gemm(int dt, const float* x, int B, int H, int W, int Cin, const float* w, const void* w16, long ldb, const float* bias,
                    const float* bias_bn, int N, float* y, long ldc, const float* residual_inplace, const ConvScratch& sc, hipStream_t s);
// y [B][H W][Cop] = conv3x3(x [B][H W][Cip]) + bias (+ tbias [B][Co]); Co of the Cop columns are written, the rest zeroed
int train_conv3x3_forward(int dt, const ConvW& c, const float* x, int B, int H, int W, const float* bias, const float* tbias, float* y,
                          const ConvScratch& sc, hipStream_t s);
// the backward of that convolution: dx [B][H W][Cip] += conv3x3(dy, wd) in place (dx == nullptr: x needs no gradient), dw [Co][Ci][3][3]
// += the gathered product dy^T x (through dwc: >= Co 9 Cip floats of scratch, compute layout), dbias [Co] and dtbias [B][Co] (or
// nullptr) += the column sums of dy
int train_conv3x3_backward(int dt, bool fixed_order, const ConvW& c, const float* x, const float* dy, int B, int H, int W, float* dx,
                           float* dwc, float* dw, float* dbias, float* dtbias, const ConvScratch& sc, hipStream_t s);

class Trainer {
 public:
  Trainer(const t2p_model_config& mc, const t2p_train_config& tc);
  ~Trainer();
  int build();
  const std::vector<TParam>& params() const { return params_; }
  long num_elements() const { return total_; }
  int load_param(const char* name, const float* host, const int64_t* shape, int ndim);
  // which: 0 parameter, 1 gradient (of the last backward pass; after a step: the clipped one), 2 EMA shadow, 3 Adam exp_avg, 4 exp_avg_sq
  int read_tensor(int which, const char* name, float* host_out);
  int write_tensor(int which, const char* name, const float* host_in);
  int set_step(int64_t step, int64_t adam_updates, int64_t ema_updates);
  int get_step(int64_t out[3]) const;
  int set_dropout_masks(const uint8_t* const* masks, int n);
  // the SDE of the loss (get_sde_loss_fn's `sde`): T2P_SDE_VE (after build), T2P_SDE_VP (std_table: host float[num_scales]) or T2P_SDE_SUBVP
  int set_sde(int sde, double beta_min, double beta_max, const float* std_table);
  // the DDIM sampler's objective instead of an SDE loss (sampler/diffusion_sampler.py:144-167): loss_type 1 = l1, 2 = l2; the two tables are
  // host float[timesteps], copied.  Before the first pass, on a trainer that was not set to VP / sub-VP; the trainer keeps it
  int set_ploss(int loss_type, int timesteps, const float* sqrt_alphas_cumprod, const float* sqrt_one_minus_alphas_cumprod);
  // block_dropout (losses.py:54-64, called at :106-107) of the NEXT loss / step / eval pass: host int32 [n][3] = (sample, start, end) and
  // the per-block decisions (host uint8 [n]) or nullptr = drawn on the device at probability p.  Consumed by that pass, then cleared
  int set_ss_blocks(const int32_t* host_blocks, int n, const uint8_t* host_drop, double p);
  // random_mask_batch (utils.py:15-60) of the NEXT loss / step / eval pass whose batch carries no mask_inpaint: host int32 [B][3] =
  // (l, lo, hi) per sample and the two mode probabilities.  That pass draws the mask on the device and consumes the request; B = 0 clears it
  int set_inpaint_draw(const int32_t* host_len_lo_hi, int B, double random_p, double contiguous_p);
  // text-context dropout of the NEXT loss / step / eval pass (training for classifier-free guidance): a dropped sample trains as if its
  // context were all zeros.  host_drop: host uint8 [B] decisions, or nullptr = drawn on the device at probability p.  B = 0 clears
  int set_context_drop(const uint8_t* host_drop, int B, double p);
  // loss_fn (losses.py:105-134); with `backward` also d loss / d parameters into the gradient buffer (zeroed first: optimizer.zero_grad())
  int loss(const t2p_train_batch& b, bool backward, bool use_ema, float* loss_host, float* score_out, hipStream_t s);
  // step_fn with train=True (losses.py:165-176) = loss(backward) + apply()
  int step(const t2p_train_batch& b, float* loss_host, hipStream_t s);
  // optimize_fn (losses.py:41-49) on the gradient buffer as it stands, state['step'] += 1, ema.update (ema.py:32-49).  Data-parallel training
  // calls loss(backward), averages grad_buffer() over the ranks (one RCCL all-reduce of the flat buffer), then this
  int apply(hipStream_t s);
  float* grad_buffer() const { return Gr_; }
  // the flat fp32 device buffers in parameters() order: which = 0 parameters, 2 EMA shadow (the numbering of read_tensor)
  int buffer(int which, float** device_ptr, int64_t* n);
  // device-to-device copies between the flat buffers on stream s, the three verbs of the reference's EMA (ema.py:51-84): 0 -> 5 store,
  // 2 -> 0 copy_to, 5 -> 0 restore.  5 is a stash allocated by the first store.  A copy into the parameters renews what the trainer
  // derives from them (prep_weights)
  int copy(int dst, int src, hipStream_t s);
  int device() const { return device_; }
  int64_t device_bytes() const { return (int64_t)pool_.held_bytes(); }

 private:
  struct Conv { long w = 0, b = 0; int Co = 0, Ci = 0, Cip = 0, Cop = 0; float* wf = nullptr; float* wd = nullptr;   // offsets into the flat buffers
                void* wf16 = nullptr; void* wd16 = nullptr; };   // 16-bit copies of wf / wd (16-bit modes, residual-block convolutions)
  struct Lin { long w = 0, b = -1; int N = 0, K = 0; bool nin = false; };
  struct Norm { long g = 0, b = 0; int C = 0, G = 0; };
  struct ResL { Norm gn0, gn1; Conv c0, c1; Lin dense, sc; bool has_sc = false; };
  struct AttnL { Norm gn; Lin nin[4]; };
  struct StL { Norm gn, ln[3]; Lin proj_in, proj_out, q1, k1, v1, o1, q2, k2, v2, o2, ff1, ff2; };
  struct LayerT { int kind = 0, in_ch = 0, out_ch = 0, up = 0, down = 0; ResL r; AttnL a; StL st; };

  long poff(const std::string& name, std::vector<int64_t> shape);
  int map_layer(const Layer& l, LayerT* out);
  int prep_weights(const float* P, hipStream_t s);
  int tg(const TGemmArgs& a);               // one strided product: launch_tgemm (F32) or launch_tgemm16 (F16 / BF16)
  int reduce_ws(long floats, float** ws);   // pass-local workspace of a fixed-order reduction; null in the f32 step (atomic form)
  int colsum(const float* dy, int nz, long rows, int N, long ld, float* out);   // out [nz][N] += column sums of dy (bias gradients)
  static ConvW conv_w(const Conv& c) { ConvW w; w.Co = c.Co; w.Ci = c.Ci; w.Cip = c.Cip; w.Cop = c.Cop; w.wf = c.wf; w.wd = c.wd;
                                       w.wf16 = c.wf16; w.wd16 = c.wd16; return w; }
  // Philox stream ids of the running loss call, all under the key tc_.seed: the diffusion times t, the noise z and the dropout mask of
  // residual block k.  philox.h tabulates them with their counter layouts and records the two known defects of this numbering, kept as they are.
  unsigned long long rng_t() const { return (unsigned long long)loss_calls_; }
  unsigned long long rng_z() const { return (unsigned long long)(loss_calls_ * 4096 + 1); }
  unsigned long long rng_dropout(int k) const { return (unsigned long long)(loss_calls_ * 4096 + 16 + k); }
  // the block-dropout decisions of the running loss call (counter = the block index); + 2 of the free ids + 2 .. + 15
  unsigned long long rng_ss() const { return (unsigned long long)(loss_calls_ * 4096 + 2); }
  // the random inpainting mask of the running loss call (counter indices: philox.h); + 3 of the free ids
  unsigned long long rng_inpaint() const { return (unsigned long long)(loss_calls_ * 4096 + 3); }
  // the context-dropout decisions of the running loss call (counter = the sample index); + 4 of the free ids
  unsigned long long rng_ctx() const { return (unsigned long long)(loss_calls_ * 4096 + 4); }
  // the integer timesteps of the running loss call under the p_loss objective (counter = the sample index); + 5 of the free ids
  unsigned long long rng_ploss_t() const { return (unsigned long long)(loss_calls_ * 4096 + 5); }

  // forward ops: each appends its backward to tape_
  TT* act(int B, int H, int W, int C, bool needs_grad = true);
  float* grad(TT* t);                       // gradient buffer of t, zero-initialised on first use
  float* tmp(size_t bytes);                 // released at the end of the call
  int linear(TT* x, const Lin& l, TT** out);
  int conv3x3(TT* x, const Conv& c, TT* tbias, TT** out);   // + bias (+ tbias [B][Co] per sample)
  int group_norm(TT* x, const Norm& n, int silu, TT** out);
  int layer_norm(TT* x, const Norm& n, TT** out);
  int attention(TT* q, TT* k, TT* v, int heads, float scale, TT** out);
  int add_scale(TT* a, TT* b, float alpha, TT** out);
  int res_block(const LayerT& L, TT* x, TT* stemb, bool train, TT** out);   // train: Dropout_0 active (eval: models/utils.py:113-115)
  int attn_block(const LayerT& L, TT* x, TT** out);
  int st_block(const LayerT& L, TT* x, TT* ctx, TT** out);
  int run_layers(const std::vector<LayerT>& ls, TT* h, TT* stemb, TT* ctx, bool train, TT** out);
  int forward_backward(const t2p_train_batch& b, const float* P, bool train, bool backward, float* loss_dev, float* score_out);
  void release();

  t2p_model_config mc_;
  t2p_train_config tc_;
  NetArch arch_;                    // the block list and the parameter table the sampling engine uses
  std::vector<TParam> params_;
  std::unordered_map<std::string, int> index_;
  long total_ = 0;
  float* P_ = nullptr;              // flat parameters
  float* Gr_ = nullptr;             // flat gradients
  float* M_ = nullptr; float* V_ = nullptr; float* E_ = nullptr;    // Adam moments, EMA shadow
  float* stash_ = nullptr;          // ema.store's copy of the parameters (buffer 5 of copy(); allocated by the first store)
  bool stashed_ = false;
  int device_ = 0;
  double* sumsq_ = nullptr;
  float* loss_dev_ = nullptr;
  float* inv_sigma_ = nullptr;
  int sde_ = T2P_SDE_VE;            // the SDE of the loss (set_sde)
  double beta_min_ = 0.0, beta_max_ = 0.0;
  float* vp_std_ = nullptr;         // VP: sqrt_1m_alphas_cumprod, float[num_scales] (the divisor of the score, models/utils.py:154)
  int ploss_ = 0;                   // the p_loss objective (set_ploss): 0 none (the SDE loss), 1 l1, 2 l2
  int ploss_T_ = 0;                 // its number of timesteps
  float* ploss_tab_ = nullptr;      // device float[2][ploss_T_]: sqrt_alphas_cumprod, then sqrt_one_minus_alphas_cumprod
  int64_t step_ = 0, adam_k_ = 0, ema_k_ = 0, loss_calls_ = 0;
  int dt_ = DT_F32;                 // compute dtype of the products
  bool plumbing16_ = false;         // the 16-bit step's plumbing (16-bit modes, or an f32 trainer created under plan switch 48): every reduction
                                    // that feeds a gradient or an update runs in a fixed order, the backward seed is scaled, apply() is guarded
  double* sumsq_part_ = nullptr;    // plumbing16_: the partial sums of the gradient norm (launch_sumsq)
  bool last_loss_finite_ = false;   // plumbing16_: the last backward pass completed with a finite loss (the overflow guard of apply)
  std::vector<std::vector<LayerT>> in_stages_, out_stages_;
  std::vector<LayerT> mid_;
  Lin pre0_, pre1_;
  Conv pre_conv_, head_conv_;
  Norm head_norm_;
  std::vector<Conv*> convs_;
  float* dwc_ = nullptr; size_t dwc_floats_ = 0;     // weight-gradient tile of the largest convolution, compute layout
  std::vector<const uint8_t*> drop_masks_;
  int drop_index_ = 0;
  // secondary-structure blocks of the next pass (set_ss_blocks): device [cap][3] int32 followed by [cap] uint8 decisions
  int* ss_blocks_ = nullptr; uint8_t* ss_drop_ = nullptr;
  int ss_cap_ = 0, ss_n_ = 0, ss_max_sample_ = -1;
  bool ss_given_ = false;           // explicit decisions (else drawn on the device at ss_p_)
  double ss_p_ = 0.0;
  int ss_pass_n_ = 0;               // the running pass: how many blocks it took over (0: none, the kernels of a pass without blocks)
  // random inpainting mask of the next pass (set_inpaint_draw): device int32 [cap][3] = (l, lo, hi)
  int* inp_llh_ = nullptr;
  int inp_cap_ = 0, inp_n_ = 0;     // inp_n_: the batch size of the request, 0 = none
  float inp_p_random_ = 0.f, inp_contig_above_ = 1.f;   // (float)random_p, (float)(1.0 - contiguous_p)
  int inp_pass_n_ = 0;              // the running pass: the request it took over (0: none, or the batch supplies mask_inpaint)
  // text-context dropout of the next pass (set_context_drop): device uint8 [cap] decisions, given or drawn by the pass
  uint8_t* ctx_drop_ = nullptr;
  int ctx_cap_ = 0, ctx_n_ = 0;     // ctx_n_: the batch size of the request, 0 = none
  bool ctx_given_ = false;          // explicit decisions (else drawn on the device at ctx_p_)
  double ctx_p_ = 0.0;
  int ctx_pass_n_ = 0;              // the running pass: the request it took over (0: none, the launches of a pass without context dropout)

  DevPool pool_;
  ConvScratch scratch_;             // pool_.get / pool_.put, for the free functions above
  hipStream_t s_ = nullptr;
  const float* Pc_ = nullptr;       // the parameters of the running pass (P_ or E_)
  std::deque<TT> acts_;
  std::vector<void*> live_;
  std::vector<std::function<int()>> tape_;
};

// the refusals of t2p_train_set_inpaint_draw / t2p_op_inpaint_mask_draw: probabilities in [0, 1] with a sum <= 1; per sample
// 0 <= l <= L and 0 <= lo < hi <= l (torch.randint(lo, hi) raises on an empty range: utils.py:34)
int check_inpaint_draw(const char* who, const int32_t* host_len_lo_hi, int B, int L, double random_p, double contiguous_p);

}  // namespace t2p

struct t2p_trainer { t2p::Trainer impl; t2p_trainer(const t2p_model_config& m, const t2p_train_config& t) : impl(m, t) {} };
