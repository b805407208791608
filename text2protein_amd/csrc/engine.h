// Score-network engine (host side, drives the HIP kernels).  The sampling loops over it: sampler.h (PC), ddim.h (DDIM).
#pragma once
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/t2p.h"
#include "t2p_kernels.h"

namespace t2p {

// Caching device allocator: exact-size free lists.  The sequence of requests of one forward pass
// is the same every evaluation, so after the first pass no hipMalloc happens (graph-capture safe).
class DevPool {
 public:
  ~DevPool();
  void* get(size_t bytes);
  void put(void* p);
  size_t held_bytes() const { return held_; }
  void* persistent(size_t bytes);  // never returned to the free lists (weights, tables)
  // Lease scope of one evaluation: every buffer taken between lease_begin and lease_end that has not been put back (or handed over
  // with keep()) by then is returned to the free lists by lease_end -- an early return anywhere inside a block cannot leave buffers
  // checked out for the lifetime of the engine.  lease_end returns how many it had to reclaim (0 on every complete evaluation).
  void lease_begin();
  int lease_end();
  void keep(void* p) { leased_.erase(p); }   // the buffer outlives the scope (cached text keys / values)
  int last_reclaimed() const { return last_reclaimed_; }
 private:
  std::multimap<size_t, void*> free_;
  std::unordered_map<void*, size_t> size_of_;
  std::vector<void*> all_;
  std::unordered_set<void*> leased_;
  int lease_depth_ = 0, last_reclaimed_ = 0;
  size_t held_ = 0;
};
// RAII form: the scope of Engine::score / Engine::set_context
struct PoolLease {
  explicit PoolLease(DevPool& p) : pool(p) { pool.lease_begin(); }
  ~PoolLease() { pool.lease_end(); }
  PoolLease(const PoolLease&) = delete;
  PoolLease& operator=(const PoolLease&) = delete;
  DevPool& pool;
};

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct ParamInfo {
  std::string name;
  std::vector<int64_t> shape;
};

struct DevLinear {      // weights [N][K] in compute dtype (+ fp32 bias)
  void* w = nullptr;
  float* b = nullptr;
  int N = 0, K = 0;     // K = taps * Cin for convolutions
  void* w_rf = nullptr;  // K = 512 projections, 16-bit modes: the row-resident GEMM's copy of w (GemmParams::Bw_rf, launch_rowres_pack)
};
struct DevNorm {
  float* gamma = nullptr;
  float* beta = nullptr;
  int C = 0, G = 0;
};

struct Layer {
  int kind = 0;  // 0 res, 1 attn, 2 st
  std::string prefix;
  int in_ch = 0, out_ch = 0, up = 0, down = 0;
  // res
  DevNorm gn0, gn1;
  DevLinear conv0, conv1, conv2;
  void* conv0_up4 = nullptr;   // up blocks, 16-bit modes: conv0 as four 2x2 phase convolutions, [4][Cout][4 * Cin] (GemmParams::Bw4)
  // blocks with a 1x1 shortcut at the block's own resolution, 16-bit modes: conv1 and the shortcut as one K loop,
  // weights [Cout][9 * Cout + Cin] and bias b1 + b2 (GemmParams::X0)
  DevLinear conv1x;
  // fragment-major copies of conv0 / conv1 (or conv1x) for the small-map convolution kernel, made at its first use
  void* fm_conv0 = nullptr; void* fm_conv1 = nullptr;
  bool has_conv2 = false;
  int temb_off = 0;
  // attn (AttnBlockpp): NIN_0|NIN_1 stacked, NIN_2, NIN_3
  DevLinear qk, v, out;
  // 16-bit modes: NIN_2 and NIN_3 as one matrix -- rows of softmax(..) sum to 1, so NIN_3(P (h W2 + b2)) = P (h W2 W3) + (b2 W3 + b3):
  // v3 = (W2 W3)^T [C][C] feeds the transposed value projection, v3.b = b2 W3 + b3 is added by the attention kernel's epilogue
  DevLinear v3;
  void* fm_qk = nullptr; void* fm_v3 = nullptr;   // C = 256: fragment-major copies of qk and v3 for attn_proj_kernel (stfuse.hip)
  // st (SpatialTransformer)
  DevLinear a1_qkv;   // 16-bit modes: to_q | to_k | to_v stacked, one projection GEMM for the self-attention
  DevLinear proj_in, proj_out, a1_qk, a1_v, a1_out, a2_q, a2_k, a2_v, a2_out, ff1, ff2;
  // 16-bit modes: the feed-forward's second Linear and proj_out as one GEMM over [g | t] (no nonlinearity between them):
  // proj_out(t + ff2(g)) = [W_po W_ff2 | W_po] [g ; t] + (W_po b_ff2 + b_po); ffpo.w = [C][4 C + C]
  DevLinear ffpo;
  // C = 256, 16-bit modes: fragment-major copies of proj_in, a1_qkv, a1_out, a2_q, a2_out, ff1 for the row-chain kernel (stfuse.hip)
  void* fm_in = nullptr; void* fm_qkv = nullptr; void* fm_out1 = nullptr; void* fm_q2 = nullptr; void* fm_out2 = nullptr; void* fm_ff1 = nullptr; void* fm_ffpo = nullptr;
  DevNorm ln1, ln2, ln3;
  void* ctx_k = nullptr;   // [B][T][C]      compute dtype (set_context)
  void* ctx_vt = nullptr;  // [B][C][Tpad]   compute dtype
};

struct Stage {
  std::vector<Layer> layers;
  int skip_ch = 0;
};

// The network's structure: the block list in execution order, the slots of the per-block time-embedding biases and the parameter
// table in the reference's parameters() order.  Shared by the sampling engine and the training step (train.cpp).
struct NetArch {
  std::vector<Stage> input_stages, out_stages;
  Stage mid_stage;
  std::vector<ParamInfo> params;
  int nf = 0, temb_dim = 0, temb_total = 0, final_ch = 0;
  int build(const t2p_model_config& c);   // checks the config
};

struct Act {  // an NHWC activation: fp32, or the compute dtype when `lowp`
  float* p = nullptr;
  int C = 0, H = 0, W = 0;
  float* cstats = nullptr;   // optional per-64-row column sums of p (GemmParams::col_stats), for the consumer's GroupNorm
  bool lowp = false;         // p holds compute-dtype (16-bit) values instead of fp32
  // optional: act(GroupNorm(p)) for the NEXT block's first norm, already produced by the split-K second pass that wrote p
  // (GemmParams::gn_out); the consumer whose norm is `pre_for` takes it (and returns it to the pool), run_stage drops it otherwise
  mutable void* pre_norm = nullptr;
  const DevNorm* pre_for = nullptr;
  int pre_silu = 0;
};
struct NormHint {            // the norm the consumer of a block's output will apply first
  const DevNorm* norm = nullptr;
  int silu = 0;
};

class Engine {
 public:
  explicit Engine(const t2p_model_config& cfg);
  ~Engine();
  int build();  // structure + parameter table (NetArch::build)
  const std::vector<ParamInfo>& params() const { return arch_.params; }
  int load_param(const char* name, const float* data, const int64_t* shape, int ndim);
  int finalize();
  // the weights from a flat fp32 device buffer in parameters() order, packed on the device (weightpack.hip); any number of times
  int load_flat(const float* device_flat, int64_t n, hipStream_t s);
  int64_t num_elements() const { return total_; }
  // the last load (either executor): bytes its packings read, bytes they wrote, how many packings (= launches of a device load) it ran
  const int64_t* load_stats() const { return load_stats_; }
  int device() const { return device_; }
  bool finalized() const { return finalized_; }
  int set_context(const float* ctx, int B, int T, hipStream_t s);
  // labels == nullptr: every row uses *step_counter (device int)
  // label_table (with step_counter): device int[num_scales], the time label of loop step i (fused sampler)
  // label_f_table (with step_counter): device float[num_scales], the fractional time label of loop step i (VP SDE)
  int score(const float* x, const int* labels, const int* step_counter, float* out, int B, hipStream_t s,
            const float* labels_f = nullptr, const int* label_table = nullptr, const float* label_f_table = nullptr);
  int64_t device_bytes() const { return (int64_t)pool_.held_bytes(); }
  int pool_reclaimed() const { return pool_.last_reclaimed(); }
  const t2p_model_config& cfg() const { return cfg_; }
  DevPool& pool() { return pool_; }
  int dtype() const { return cfg_.compute_dtype; }

 private:
  // the one walk that places and fills every weight-derived buffer; run by finalize() (host executor) and load_flat() (device executor)
  int pack_weights();
  int dest(void** slot, size_t bytes);
  const float* psrc(const std::string& name, int64_t numel);
  int pack(int kind, void* dst, int64_t off, int dtype, std::initializer_list<const float*> srcs, std::initializer_list<int64_t> dims);
  int pack_frag(void** slot, const void* w, int N, int K);
  int pack_rowres(DevLinear* l);
  int pack_linear(const std::string& wname, const std::string& bname, int N, int K, DevLinear* out,
                  bool conv3x3 = false, bool nin = false, int force_dtype = -1, int cin_pad = 0);
  int pack_stack2(const std::string& w0, const std::string& b0, const std::string& w1, const std::string& b1,
                  int N, int K, bool nin, bool has_bias, DevLinear* out);
  int pack_norm(const std::string& prefix, int C, int G, DevNorm* out);

  int run_stage(Stage& st, Act& h, const Act* skip, int B, hipStream_t s, const Layer* next_after = nullptr);
  int res_block(Layer& L, const Act& x, const Act* skip, Act* out, int B, hipStream_t s, NormHint hint = NormHint());
  int attn_block(Layer& L, const Act& x, Act* out, int B, hipStream_t s);
  int st_block(Layer& L, const Act& x, Act* out, int B, hipStream_t s);
  int group_norm(const Act& x, const Act* x1, const DevNorm& n, float eps, int silu, int down, int B, void** out,
                 hipStream_t s, void** raw_out = nullptr);
  int gemm(GemmParams& p, hipStream_t s);
  int attach_ws(GemmParams& p);
  // gemm() that also produces the output's GroupNorm column statistics when the kernel can (else *cstats = null)
  int gemm_stats(GemmParams& p, float** cstats, hipStream_t s);
  void free_act(Act& a) { pool_.put(a.p); pool_.put(a.cstats); pool_.put(a.pre_norm); a.p = nullptr; a.cstats = nullptr; a.pre_norm = nullptr; }
  void drop_pre_norm(const Act& a) { pool_.put(a.pre_norm); a.pre_norm = nullptr; }
  int attention(const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, int B,
                int heads, int nq, int nk, int d, float scale, hipStream_t s);
  int linear(const void* a, bool a_is_f32, const DevLinear& w, long rows, void* c, bool c_f32, const float* residual,
             float alpha, hipStream_t s, bool use_bias = true, float** cstats = nullptr, bool r_lowp = false);
  // the residual stream between blocks is stored in the compute dtype (f16 mode only): halves the HBM-bound
  // traffic of GroupNorm-apply and of the residual / output halves of the block-closing GEMM epilogues
  bool res_lowp() const { return g_plan.lowp_residual && cfg_.compute_dtype == DT_F16; }

  t2p_model_config cfg_;
  NetArch arch_;
  std::unordered_map<std::string, HostTensor> host_;
  bool finalized_ = false;
  DevPool pool_;
  std::unordered_map<std::string, std::pair<int64_t, int64_t>> poff_;   // parameter name -> (offset, element count) in a flat buffer
  int64_t total_ = 0;
  int device_ = 0;
  const float* flat_ = nullptr;        // the running load: the flat device buffer (load_flat) or null (finalize: host_)
  hipStream_t pack_stream_ = nullptr;
  int64_t load_stats_[3] = {0, 0, 0};

  int cpad_ = 8;                // channel padding of the network input
  DevLinear pre0_, pre1_, pre_conv_, head_conv_, dense_all_;
  DevNorm head_norm_;
  float* pre_conv_direct_ = nullptr;   // [nf][9][C] fp32 weights of the direct input convolution
  void* pre_conv_split_ = nullptr;     // the same, each weight as two f16 terms (pre_conv_split_kernel; 16-bit modes)
  float* inv_sigma_ = nullptr;  // [N] fp32, 1 / sigmas[label] (descending sigmas)
  float* unit_scale_ = nullptr; // [N] fp32 ones: the output scale without scale_by_sigma
  int ctx_B_ = 0, ctx_T_ = 0, ctx_Tpad_ = 0;   // ctx_B_ == 0: no valid projection (never set, or the weights changed since)
  int ctx_cap_B_ = 0, ctx_cap_T_ = 0;          // the shape the per-layer key / value buffers were allocated for
  void* splitk_ws_ = nullptr;
  size_t splitk_ws_bytes_ = 0;
  const float* tb_ = nullptr;   // per-eval temb biases [R][arch_.temb_total]
  long tb_ld_ = 0;
};

}  // namespace t2p

struct t2p_engine { t2p::Engine impl; explicit t2p_engine(const t2p_model_config& c) : impl(c) {} };
