// Launchers for the non-GEMM kernels of the score network and the SDE update.
#pragma once
#include "t2p_common.h"

namespace t2p {

// ---- GroupNorm (reference nn.GroupNorm, layers.py:282,292; attention.py:77; ncsnpp.py:214) ----
// x is NHWC fp32, optionally the channel-concat of two sources.  stats = [B][G][2] (mean, rstd).
struct GroupNormArgs {
  const float* x0 = nullptr; const float* x1 = nullptr;
  int C0 = 0, C1 = 0;
  int B = 0, HW = 0;       // input pixels per sample
  int G = 0;
  float eps = 1e-6f;
  int lowp_dtype = DT_F32;   // DT_F16 / DT_BF16: x0 (and x1) hold 16-bit values
  float* partial = nullptr;  // workspace [B][nchunk][G][2], nchunk = gn_num_chunks(HW)
  float* stats = nullptr;    // [B][G][2]
};
int gn_num_chunks(int HW);
int launch_gn_stats(const GroupNormArgs& a, hipStream_t s);

// statistics from per-chunk column sums written by the GEMM epilogue (GemmParams::col_stats):
// cs0 / cs1 = [B * HW / 64][C0 or C1][2] for the two channel-concatenated sources
int launch_gn_finalize_cols(const float* cs0, const float* cs1, int C0, int C1, int B, int HW, int G, float eps,
                            float* stats, hipStream_t s);

struct GroupNormApplyArgs {
  const float* x0 = nullptr; const float* x1 = nullptr;
  int C0 = 0, C1 = 0, B = 0, H = 0, W = 0, G = 0;
  const float* stats = nullptr;       // [B][G][2]
  const float* gamma = nullptr; const float* beta = nullptr;
  int silu = 0;
  int down = 0;                        // 2x2 mean of the activated map (layers.py:185-188)
  void* out = nullptr;                 // [B][H'*W'][C] in `dtype`
  int dtype = DT_F32;
  int x0_lowp = 0;                     // x0 is stored in `dtype` (16-bit) instead of fp32 (single source only)
  void* raw_out = nullptr;             // optional: un-normalised x (concat of both sources) in `dtype`,
                                       // same resolution as the input (not with `down`)
  float eps = 0.f;                     // launch_gn_small / launch_gn_apply_cols only
  const float* cs0 = nullptr; const float* cs1 = nullptr;   // launch_gn_apply_cols: column statistics of the two sources
};
int launch_gn_apply(const GroupNormApplyArgs& a, hipStream_t s);
// 16-bit maps of <= 4096 pixels whose statistics arrive as per-64-row column sums (GEMM epilogues): finalize and apply in ONE
// launch -- a block owns a 64-channel slab (whole groups) of one sample, folds the slab's column sums itself, then normalises
bool gn_apply_cols_eligible(const GroupNormApplyArgs& a);
int launch_gn_apply_cols(const GroupNormApplyArgs& a, hipStream_t s);
// statistics + normalisation (+SiLU, + raw copy) of a small map in ONE launch (no `stats` input, no `down`)
bool gn_small_eligible(const GroupNormApplyArgs& a);
int launch_gn_small(const GroupNormApplyArgs& a, hipStream_t s);

// ---- LayerNorm over the last axis (attention.py:203-205), eps 1e-5 ---------------------------
int launch_layernorm(const float* x, const float* gamma, const float* beta, void* out, int dtype,
                     long rows, int C, float eps, hipStream_t s, int x_lowp = 0);

// ---- row softmax: P[r][0:n] = softmax(scale * S[r][0:n]); P[r][n:ldp] = 0 ----------------------
int launch_softmax(const float* S, long lds, void* P, long ldp, int dtype, long rows, int n, float scale,
                   hipStream_t s);

// ---- GEGLU (attention.py:37-44): out[r][j] = u[r][j] * gelu_erf(u[r][inner + j]) ----------------
int launch_geglu(const float* u, void* out, int dtype, long rows, int inner, hipStream_t s, int interleaved = 0);

// ---- 2x2 mean pooling of an NHWC fp32 map (skip branch of a down block, layers.py:309-311) ------
int launch_pool2x2(const float* x, void* out, int dtype, int B, int H, int W, int C, hipStream_t s, int x_lowp = 0);

// ---- pre_conv: 3x3, C in {5, 8} NCHW fp32 -> nf NHWC (fp32 or a 16-bit out_dtype); w = [9][C][nf] fp32 (tap-major, output channel contiguous) --
int launch_pre_conv(const float* x, const float* w, const float* bias, void* out, int out_dtype, int B, int C, int H, int W, int nf,
                    hipStream_t s, float* cstats = nullptr);
bool pre_conv_fuses_col_stats(int W, int nf);
// the same layer on the 16-bit matrix pipe with every fp32 operand split into two f16 terms (fp32-class accuracy, plan switch 38):
// wsplit = the weights in that form (pre_conv_split_weight_bytes bytes, written by launch_pre_conv_split_weights from w [9][C][nf])
size_t pre_conv_split_weight_bytes(int C, int nf);
bool pre_conv_split_ok(int out_dtype, int C, int H, int W, int nf);
int launch_pre_conv_split_weights(const float* w, void* wsplit, int C, int nf, hipStream_t s);
int launch_pre_conv_split(const float* x, const void* wsplit, const float* bias, void* out, int out_dtype, int B, int C, int H, int W, int nf,
                          hipStream_t s, float* cstats = nullptr);

// ---- NCHW fp32 (B,C,L,L) -> NHWC fp32 [B][L*L][Cpad], zero padded channels -----------------------
int launch_nchw_to_nhwc(const float* x, float* out, int B, int C, int HW, int Cpad, hipStream_t s);

// ---- time embedding ------------------------------------------------------------------------------
// emb[r][:] = [sin(t f_k) | cos(t f_k)] (layers.py:97-111); label of row r = labels ? labels[r]
// : *step_counter (device scalar) -- the sampler advances a device-side counter so that a
// captured graph of one PC step can be replayed.
// labels_f (optional): fractional time values for the embedding (VP path: labels = t * (N - 1),
// reference models/utils.py:150-152); the sigma lookup always uses the integer labels
// label_table (optional, with step_counter): the label is label_table[*step_counter] instead of *step_counter
// label_f_table (optional, with step_counter): fractional label of loop step i (VP SDE in the fused sampler)
int launch_timestep_embedding(const int* labels, const float* labels_f, const int* step_counter, float* emb, int rows,
                              int dim, hipStream_t s, const int* label_table = nullptr, int n_table = 0, const float* label_f_table = nullptr);
// out[r][n] = bias[n] + sum_k act(in[r][k]) * W[n][k]   (fp32; act = SiLU when silu != 0)
int launch_small_linear(const float* in, const float* W, const float* bias, float* out, int rows, int K, int N,
                        int silu, hipStream_t s);

// grid of an elementwise launch: one thread per item up to 16384 blocks, grid-stride loops cover the rest
static inline int ew_grid(long total, int block = 256) {
  long g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

// ---- reverse-diffusion predictor + Langevin corrector (sampling.py:157-199) ------------------------
// One set of kernels for the plain and the guided loop, under the VE and the VP SDE.  The score every kernel reads is formed per
// element, s = scale (w o_c + w1 o_u) (classifier-free guidance, reference sampler/diffusion_sampler.py:128): each product and sum
// of the guidance sum rounds to float32 in this order, then the scale multiplies.  o_u null: s = scale o_c; with scale == 1 that is
// the network output itself.  The rest of each update states its rounding too: x_mean of the predictor is two rounded products and
// their sum, the Langevin update and both noise terms are FMAs (update_loop.h, kernels.hip).
struct GuidedScore {
  const float* o_c = nullptr;          // network output (under the text context)
  const float* o_u = nullptr;          // under the zero context; null = no guidance sum
  float w = 1.f, w1 = 0.f;             // guidance weight and (float)(1 - w) as the reference rounds it (from the double)
  float scale = 1.f;                   // VE: 1; VP: -1 / std of the step's label (models/utils.py:153-157) ...
  const float* scale_table = nullptr;  // ... or scale_table[*step_counter]
  const int* step_counter = nullptr;   // device step index of every per-step table (scale, alpha, G, x_coef)
  int n_table = 0;
};
struct SdeUpdateArgs {
  const float* x = nullptr;        // current state (B, C, L, L) fp32
  const float* noise = nullptr;    // standard normal draws
  const unsigned char* mask = nullptr;  // conditional_mask (1 = free); null together with x_initial
  const float* x_initial = nullptr;
  float* x_out = nullptr;
  float* x_mean_out = nullptr;     // un-masked x_mean (masking of the final x_mean: sampling.py:287)
  long n = 0;                      // total elements
};
// Replacement inpainting (reference score_sde_pytorch/inpainting.py:39-47): after an update U the known region is overwritten with the
// data noised to the step's level, r = fl(fl(a d) + fl(z s)), and x_mean becomes known ? fl(a d) : the new x.  An element the
// condition mask freezes stays x_initial (in x and in x_mean).  Rides in the update kernels: no launch of its own.
struct InpaintReplace {
  const unsigned char* known = nullptr;   // 1 = known (B, C, L, L); null together with data
  const float* data = nullptr;            // the clean data d, fp32
  const float* noise = nullptr;           // z; null = drawn in the kernel: sampling layout, (seed, stream), counter = quad q
  const float* mean_table = nullptr;      // a of loop step i, read at *step_counter ...
  const float* std_table = nullptr;       // ... and s; both null: mean_coef / std below
  const int* step_counter = nullptr;      // device step index: the tables' row and the step word of the draw; null: `step`
  int n_table = 0;
  float mean_coef = 1.f, std = 0.f;
  unsigned long long seed = 0, stream = 0;
  unsigned int step = 0;
};
// sums[0] = sum_b ||s_b||_2, sums[1] = sum_b ||noise_b||_2  (per-sample norms over B samples, summed over b).  width: consecutive
// elements a thread sums per trip, 1 (the plain loop and t2p_op_langevin*) or 4 (the guided loop): the order of the float32 sums
int launch_langevin_norms(const GuidedScore& g, const float* noise, int B, long per_sample, float* sq_ws, float* sums, int width,
                          hipStream_t s);
// corrector: step = (snr * mean_norm_noise / mean_norm_grad)^2 * 2 * alpha, with the two means
// = sums[] / batch_total (batch_total may exceed the local batch: global-batch semantics)
// alpha_table (optional): alpha = alpha_table[*step_counter] (VP: sde.alphas[timestep], sampling.py:184-186)
// x_out2 (optional): a second copy of the new state, the other half of the [x ; x] input of the next guided evaluation
// r (optional, here and in the predictor): the replacement of the known region after the update
int launch_langevin_update(const SdeUpdateArgs& a, const GuidedScore& g, float* x_out2, const float* sums, float batch_total,
                           float snr, float alpha, hipStream_t s, const float* alpha_table = nullptr, const InpaintReplace* r = nullptr);
// predictor: x_mean = x_coef x + G^2 * s * (0.5 if probability_flow); x = x_mean + (0 if pf else G) z
// G = G_table[*step_counter] when G_table != null, else G_value
// x_coef_table (optional, with G_table): VP, 2 - sqrt(alpha) (sde_lib.py:148-157); x_coef_value: the coefficient where no table is given
int launch_predictor_update(const SdeUpdateArgs& a, const GuidedScore& g, float* x_out2, const float* G_table, float G_value,
                            int probability_flow, hipStream_t s, const float* x_coef_table = nullptr, float x_coef_value = 1.f,
                            const InpaintReplace* r = nullptr);
// noise[i] = N(0,1) from Philox4x32-10 keyed by (seed, stream); counter = element index / 4
int launch_philox_normal(float* out, long n, unsigned long long seed, unsigned long long stream,
                         const int* step_counter, hipStream_t s);
int launch_add_int(int* counter, int delta, hipStream_t s);
int launch_scale(float* x, long n, float a, hipStream_t s);

// ---- fused attention (attention.hip): 16-bit dtypes, head dim 32 / 64 / 128 -------------------------
bool attention_flash_eligible(int dtype, int d, long ldq, long ldk, long ldvt, long ldo);
int launch_attention_flash(int dtype, const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt,
                           void* out, int B, int heads, int nq, int nk, int d, float scale, hipStream_t s, bool v_rowmajor = false);

// ---- single-head attention with a wide head (AttnBlockpp, layers.py:160-176): d = 256 / 512 / 1024, n <= 1024, one launch --------
bool attention_strip_eligible(int dtype, int heads, int nq, int nk, int d, long ldq, long ldk, long ldvt, long ldo);
// optional epilogue: out = alpha (attention + bias[channel] + residual[query][channel]), stored fp32 or in the compute dtype, with
// the per-64-query column sums / sums of squares of the stored fp32 values (col_stats [B n / 64][d][2], n % 64 == 0)
struct StripEpilogue {
  const float* bias = nullptr;
  const void* residual = nullptr;
  int r_lowp = 0;
  long ldr = 0;
  float alpha = 1.f;
  int out_f32 = 0;
  float* col_stats = nullptr;
  int frag_major = 0;      // k and vt are fragment-major [B][n d] (GemmParams::c_frag of their projections; attention_strip_frag_major_ok)
};
bool attention_strip_frag_major_ok(int dtype, int n, int d);
int launch_attention_strip(int dtype, const void* q, long ldq, const void* k, long ldk, const void* vt, long ldvt, void* out, long ldo,
                           int B, int n, int d, float scale, hipStream_t s, const StripEpilogue* ep = nullptr);

// ---- 3x3 convolution of the 8x8 / 4x4 levels + the GroupNorm (+SiLU) that follows, one launch (smallconv.hip) ----------------------
// out[row][n] = alpha (sum_{tap, c} A[pixel(row, tap)][c] Wt[n][tap C + c] + sum_c X[row][c] Wt[n][9 C + c] + bias[n]
//                      + bias_bn[sample][n] + R[row][n]);   normed = act(GroupNorm(out))
struct SmallConvArgs {
  int dtype = DT_F16;
  const void* A = nullptr;      // [B H W][C]     16-bit, dense
  int B = 0, H = 0, W = 0, C = 0, N = 0;
  const void* Wt = nullptr;     // [N][ldw]       16-bit, K index = tap * C + c, then the shortcut columns
  long ldw = 0;
  int w_fm = 0;                 // Wt is the fragment-major copy of the [N][ldw] matrix (launch_sf_frag_major; ldw % 32 == 0)
  const void* X0 = nullptr; const void* X1 = nullptr;   // optional shortcut sources [B H W][CX0], [B H W][CX1] (16-bit, dense)
  int CX0 = 0, CX1 = 0;
  const float* bias = nullptr;      // [N]
  const float* bias_bn = nullptr;   // [B][ld_bn] (time-embedding bias)
  long ld_bn = 0;
  const void* R = nullptr;          // residual [B H W][N], 16-bit
  float alpha = 1.f;
  void* out = nullptr;              // raw result [B H W][N], fp32 (out_f32) or 16-bit; may be null when `normed` is wanted only
  int out_f32 = 0;
  float* col_stats = nullptr;       // [B H W / 64][N][2] column sums / sums of squares of the raw fp32 values (8x8 maps)
  void* normed = nullptr;           // act(GroupNorm(out)) [B H W][N], 16-bit; null = no norm
  const float* gn_gamma = nullptr; const float* gn_beta = nullptr;
  int groups = 0, gn_silu = 0;
  float gn_eps = 1e-6f;
};

// ---- row-block chains of a SpatialTransformer block in one launch (stfuse.hip; plan switch 39) -------------------------------------
// st_entry: a = GroupNorm(x) -> t = proj_in(a) + b -> LayerNorm_1(t) -> q | k | v  (model/attention.py:250-256, 208-213, 170-176)
struct StEntryArgs {
  int dtype = DT_F16;
  int B = 0, n = 0, C = 0;               // samples, tokens per sample (H W), channels
  const void* x = nullptr;               // [B n][C] 16-bit: the block input (raw with cstats, already normalised without)
  const float* cstats = nullptr;         // per-64-row column sums of x ([B n / 64][C][2]) or null
  const float* gn_gamma = nullptr; const float* gn_beta = nullptr; int groups = 0; float gn_eps = 1e-6f;
  // the two weight matrices are FRAGMENT-MAJOR copies (launch_sf_frag_major of the row-major [N][K] 16-bit matrices)
  const void* w_in = nullptr; const float* b_in = nullptr;       // proj_in [C][C] 16-bit, bias [C]
  const float* ln_gamma = nullptr; const float* ln_beta = nullptr; float ln_eps = 1e-5f;
  const void* res = nullptr;             // optional [B n][C] 16-bit residual of the first product (may be `t` itself: rows are private)
  const void* w_qkv = nullptr;           // [n2][C] 16-bit: to_q | to_k | to_v stacked (n2 = 3 C), or one projection (n2 = C); no bias
  int n2 = 0;
  const float* b2 = nullptr;             // optional bias of the second product [n2]
  int geglu = 0;                         // n2 = 8 C interleaved (value, gate) columns -> out2 [B n][n2 / 2] = value * gelu_erf(gate)
  // optional third product (with geglu): y = [out2 | t] W_3^T + b_3 + res3: w3 [C][5 C] fragment-major, res3 / y [B n][C] 16-bit;
  // out2 then stays on chip (qkv unused).  y_stats: per-64-row column sums of y, ACCUMULATED (zeroed beforehand: `zero` of an earlier launch)
  const void* w3 = nullptr; const float* b3 = nullptr; const void* res3 = nullptr; void* y = nullptr; float* y_stats = nullptr;
  float* zero = nullptr; long zero_n = 0;   // optional: this launch zeroes zero[0 .. zero_n)
  void* t = nullptr;                     // out [B n][C] 16-bit: the block's residual stream
  void* qkv = nullptr;                   // out [B n][n2] 16-bit
};
// the projections of an AttnBlockpp in one launch (C = 256): GroupNorm apply -> q | k (row-major [B n][2 C], + bias) and the merged
// value projection written transposed (vt [B][C][npad]); weights fragment-major (launch_sf_frag_major); x / cstats as in StEntryArgs
struct AttnProjArgs {
  int dtype = DT_F16;
  int B = 0, n = 0, C = 0;
  long npad = 0;
  const void* x = nullptr; const float* cstats = nullptr;
  const float* gn_gamma = nullptr; const float* gn_beta = nullptr; int groups = 0; float gn_eps = 1e-6f;
  const void* w_qk = nullptr; const float* b_qk = nullptr;     // [2 C][C], bias [2 C]
  const void* w_v = nullptr;                                   // [C][C] (no bias: the attention kernel's epilogue adds it)
  void* qk = nullptr; void* vt = nullptr;
  void* k_fm = nullptr;      // optional: the k half goes here FRAGMENT-MAJOR ([B][n C]) and vt is written fragment-major as well (npad == n):
                             // the operands of attn_strip_kernel<.., FM> (attention_strip_frag_major_ok)
};
bool attn_proj_eligible(const AttnProjArgs& a);
int launch_attn_proj(const AttnProjArgs& a, hipStream_t s);
bool st_entry_eligible(const StEntryArgs& a);
int launch_st_entry(const StEntryArgs& a, hipStream_t s);
// out = W [N][K] (16-bit, row-major) re-ordered so that every MFMA fragment of 16 rows x 32 K is 1 KiB contiguous (same size)
int launch_sf_frag_major(int dtype, const void* W, void* out, int N, int K, hipStream_t s);
// ---- row-resident GEMM for the K = 512 projections (rowgemm.hip; plan switch 49, gemm_rowres_eligible in t2p_common.h) ---------------
// p.Bw_rf = the copy launch_rowres_pack made of the weights: piece (slice s, 32-deep step t, column tile j, lane l) of 16 bytes at
// (((s 16 + t) 4 + j) 64 + l) 16 holds W[64 s + hperm(16 j + l % 16)][32 t + 8 (l / 16) .. + 8) -- what lane l feeds the MFMA
int launch_gemm_rowres(const GemmParams& p, hipStream_t s);
const char* gemm_rowres_kernel_name(int dtype);
int launch_rowres_pack(int dtype, const void* W, long ldb, void* out, int N, hipStream_t s);   // W [N][ldb] 16-bit, K = 512; out N x 512
bool small_conv_eligible(const SmallConvArgs& a);
int launch_small_conv_gn(const SmallConvArgs& a, hipStream_t s);

int launch_convert(const float* in, void* out, int dtype, long n, hipStream_t s);
int launch_widen(const void* in, int dtype, float* out, long n, hipStream_t s);   // compute dtype -> fp32
int launch_gather_label(const int* labels, const int* step_counter, const float* table, float* out, int B, int N,
                        hipStream_t s, const int* label_table = nullptr);
int launch_apply_mask(float* x, const unsigned char* mask, const float* x_initial, long n, hipStream_t s);
// x = where(known, data, x): the start of a replacement-inpainting run (inpainting.py:66)
int launch_put_known(float* x, const unsigned char* known, const float* data, long n, hipStream_t s);
int launch_decode6d(const float* x, int B, int C, int L, float* clipped, float* absval, int* lengths, hipStream_t s);
// 6D encode of a padded batch of backbones (dataset.py:396-450, :200-239, :114-168): xyz [B][L][3][3] fp32 (N, Ca, C), nres [B],
// atom_ok [B][L][3] or null -> coords_6d [B][C][L][L] (C = 5 or 8), mask_pair [B][L][L]; blocks [n][4] / pairs [npairs][2]: device
// copies of the secondary-structure blocks and of the ordered block pairs of one sample each (ss_constraints_kernel)
int launch_encode6d(const float* xyz, const int* nres, const unsigned char* atom_ok, int B, int C, int L, const int* blocks, const int* pairs,
                    int npairs, float* coords_6d, unsigned char* mask_pair, hipStream_t s);
int launch_embedding_gather(const void* table, int dtype, const int* ids, float* out, long ntok, int dim, int vocab, int* bad, hipStream_t s);
// Byte offsets into a caller's workspace, every part 256-byte aligned (FoldWorkspace, RefineWorkspace, RoundsWorkspace).
struct WorkspaceCarve {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t at = total;
    total += (bytes + 255) / 256 * 256;
    return at;
  }
};
// ---- after the decode: backbones from the maps (fold.hip) ----
// absval / lengths as launch_decode6d writes them -> xyz [B][L][3][3] (N, CA, C), status [B] (0 ok, 1 degraded, -1 improper mask),
// placed [B][L] (1 = residue without a frame of its own), diag [B][16] double.  The geodesic matrix of a chain stays in LDS up to
// FOLD_LDS_MAX residues per map side and lives in the workspace above; FOLD_MAX_L bounds the coordinate arrays kept in LDS.
constexpr int FOLD_LDS_MAX = 128, FOLD_MAX_L = 512;
long fold6d_workspace_bytes(int B, int L);           // -1 when L is out of range
int launch_fold6d(const float* absval, const int* lengths, int B, int L, float known_below, int stress_steps, float dist_std, float angle_std_deg,
                  float* xyz, int* status, unsigned char* placed, double* diag, void* workspace, long workspace_bytes, hipStream_t s);
// the four restraint sums and their counts of given backbones: out[b * stride + 0..7] (double)
int launch_restraint_score(const float* xyz, const float* absval, const int* lengths, int B, int L, float dist_std, float angle_std_deg,
                           double* out, int stride, void* workspace, long workspace_bytes, hipStream_t s);

// ---- secondary structure of CA traces: P-SEA (sse.hip) ----
// xyz [B][L][atoms][3] fp32 (atoms = 3: atom 1 is read; atoms = 1: a CA trace), len [B], atom_ok [B][L][atoms] or null, target [B][L]
// letters or null -> letters [B][L] ('a' / 'b' / 'c', 0 past the length), counts [B][12], status [B].  One workgroup per chain; SSE_MAX_L
// (= FOLD_MAX_L) bounds the trace and the flags it keeps in LDS.
constexpr int SSE_MAX_L = FOLD_MAX_L;
int launch_annotate_sse(const float* xyz, const int* len, const unsigned char* atom_ok, int B, int L, int atoms, const unsigned char* target,
                        unsigned char* letters, int* counts, int* status, hipStream_t s);

// ---- refinement of folded backbones against the restraint set (refine.hip) ----
// One workgroup per chain, a persistent staged L-BFGS in double; REFINE_MAX_L bounds the five coordinate-sized vectors a workgroup keeps
// in LDS (18 KB each at 256 residues) and is every shipped data.max_res_num, like TM_MAX_L.  A stage is six doubles on the host:
// sep_lo, sep_hi, w_dist, w_ang, w_rep, max_iter.
constexpr int REFINE_MAX_L = 256, REFINE_MAX_STAGES = 8;
long refine_workspace_bytes(int B, int L);           // -1 when L is out of range
int launch_refine_backbone(const float* xyz_in, const float* absval, const int* lengths, int B, int L, const double* schedule, int n_stages,
                           float dist_std, float angle_std_deg, float arm_min_deg, float* xyz_out, int* status, double* diag, void* workspace,
                           long workspace_bytes, hipStream_t s);
// one evaluation of the same energy: out9 [B][9] (eight unweighted terms, weighted total), grad [B][L][3][3], both double
int launch_restraint_energy(const float* xyz, const float* absval, const int* lengths, int B, int L, const double* stage6, float dist_std,
                            float angle_std_deg, float arm_min_deg, double* out9, double* grad, void* workspace, long workspace_bytes,
                            hipStream_t s);
// the same two kernels over B candidates that share maps: every candidate has its own coordinates and its own entry of lengths, and
// candidate c reads the maps of chain c / group (absval holds B / group chains; the workspace is that of B chains).  A length below 2
// leaves a candidate out (status -1, zeros).  grad may be null.  group = 1 is the two launchers above.
int launch_refine_grouped(const float* xyz_in, const float* absval, const int* lengths, int B, int group, int L,
                          const double* schedule, int n_stages, float dist_std, float angle_std_deg, float arm_min_deg, float* xyz_out,
                          int* status, double* diag, void* workspace, long workspace_bytes, hipStream_t s);
int launch_restraint_energy_grouped(const float* xyz, const float* absval, const int* lengths, int B, int group, int L, const double* stage6,
                                    float dist_std, float angle_std_deg, float arm_min_deg, double* out9, double* grad, void* workspace,
                                    long workspace_bytes, hipStream_t s);

// ---- refinement in rounds (refine_rounds.hip) ----
// The phi / psi move on N / CA / C chains held in Cartesian coordinates, and the loop perturb -> minimise -> select of rosetta_min/run.py
// on the device: per round one move launch, one refine launch over batch x replicas workgroups, one energy launch, one selection launch.
constexpr int REFINE_MAX_ROUNDS = 8, REFINE_MAX_REPLICAS = 16, REFINE_STREAM_STRIDE = 16;
// in_status (may be null): a chain whose entry is neither 0 nor 1 keeps it; cand_lengths (may be null): [B][replicas], the chain's length
// for a candidate that was written and -1 for one that was refused -- what launch_refine_grouped takes
int launch_perturb_torsions(const float* xyz_in, const int* lengths, const int* chain_ids, const int* in_status, int B, int L, int replicas,
                            float amp_deg, unsigned long long seed, unsigned long long stream, int keep_first, float* xyz_out, int* status,
                            int* cand_lengths, hipStream_t s);
long refine_rounds_workspace_bytes(int B, int L, int replicas);      // -1 when L or replicas is out of range
int launch_refine_rounds(const float* xyz_in, const float* absval, const int* lengths, const int* chain_ids, int B, int L,
                         const double* schedules, int rounds, int n_stages, int replicas, const double* select_stage, float amp_deg,
                         unsigned long long seed, unsigned long long stream_base, float dist_std, float angle_std_deg, float arm_min_deg,
                         float* xyz_out, int* status, double* diag, double* trace, void* workspace, long workspace_bytes, hipStream_t s);

// ---- scoring folded backbones: TM-align (tmalign.hip) ----
// The default path of the reference's tm/TMalign.cpp for pairs of CA traces: xyz_* [n][L][atoms][3] fp32 (atoms = 3: N / CA / C, atom 1
// is read; atoms = 1: a CA trace), len_* [n]; pairs [n_pairs][2] or null = all n_a x n_b pairs, row-major.  One workgroup per pair.
// out8 [n_pairs][8] double, b2a [n_pairs][Lb] (or null), rot12 [n_pairs][12] (or null), status [n_pairs].  TM_MAX_L is every shipped
// data.max_res_num: it bounds the registers a lane holds (TM_MAX_L / 64 residues) and the LDS of a workgroup.
constexpr int TM_MAX_L = 256;
long tm_align_workspace_bytes(int n_pairs, int La, int Lb);          // -1 when La or Lb is out of range
int tm_align_info(int La, int Lb, int* out4);     // wavefronts and dynamic LDS bytes of a workgroup; the kernel's registers and scratch
int launch_tm_align(const float* xyz_a, const int* len_a, int n_a, int La, int atoms_a, const float* xyz_b, const int* len_b, int n_b, int Lb,
                    int atoms_b, const int* pairs, int n_pairs, double* out8, int* b2a, double* rot12, int* status, void* workspace,
                    long workspace_bytes, hipStream_t s);

// ---- weight packing on the device (weightpack.hip) -----------------------------------------------------------------------------
// One packing = one kind applied to fp32 sources, written to dst in `dtype`.  Engine::pack_weights decides which packings a network
// needs; the host load path runs them through weight_pack_host (engine.cpp), the device refresh through launch_weight_pack: same bits.
//   kind        sources                          d[]                          writes
//   WP_COPY     up to three vectors              n0, n1, n2                   src0 | src1 | src2 (Linear, 1x1, norms, biases, stacks)
//   WP_ROWS     (rows, rowlen)                   rows, rowlen, ld             dst[r ld + j]
//   WP_CONV3    (N, Ci, 3, 3)                    N, Ci, cin_pad, ld           dst[n ld + tap cin_pad + c], channels past Ci zero
//   WP_CONV3_T  (N, C, 3, 3)                     N, C                         dst[(tap C + c) N + n]
//   WP_NIN      one or two (K, N)                K, N, nsrc                   dst[z N K + n K + k]
//   WP_GEGLU    (2 inner, rowlen)                inner, rowlen                rows interleaved (value_j, gate_j)
//   WP_UP4      (co, ci, 3, 3)                   co, ci                       dst[((ph co + n) 4 + tap) ci + c], taps summed in (kh, kw) order
//   WP_ADD      a, b                             n                            a + b (fp32)
//   WP_PRODUCT  A (M, K), B (K, N), [addv (N)]   M, K, N, transposed, ld      sum_k A B (+ addv): fp32, ascending k, product and add rounded
//   WP_DOT64    W (N, K), v (K), b0 (N)          N, K                         (float)(b0[n] + sum_j (double) W[n][j] v[j])
// A pitch (ld) or cin_pad of 0 means "dense".
enum { WP_COPY = 0, WP_ROWS = 1, WP_CONV3 = 2, WP_CONV3_T = 3, WP_NIN = 4, WP_GEGLU = 5, WP_UP4 = 6, WP_ADD = 7, WP_PRODUCT = 8, WP_DOT64 = 9 };
struct WeightPack {
  int kind = WP_COPY;
  const float* src[3] = {nullptr, nullptr, nullptr};
  void* dst = nullptr;
  int64_t d[6] = {0, 0, 0, 0, 0, 0};
  int dtype = DT_F32;
};
// checks p, fills in defaulted pitches; the packing writes the block [rows][width] at pitch ld (elements of dtype)
int weight_pack_shape(WeightPack& p, int64_t* rows, int64_t* width, int64_t* ld);
int launch_weight_pack(const WeightPack& p, hipStream_t s);
void weight_pack_bytes(const WeightPack& p, int64_t rows, int64_t width, int64_t* bytes_read, int64_t* bytes_written);

}  // namespace t2p
