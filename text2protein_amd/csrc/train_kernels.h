// Launchers of the TRAINING step's kernels (train_kernels.hip): the backward halves of the score network's operators, the
// denoising score-matching loss and the optimizer / EMA updates (reference score_sde_pytorch/losses.py:26-186,
// score_sde_pytorch/models/ema.py:32-49).  Everything in memory is fp32; the products run on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32, launch_tgemm) or on the 16-bit matrix pipe (launch_tgemm16): SURVEY.md 8(f)4.  Every gradient output
// ACCUMULATES (+=) into its destination unless stated.
// Each reduction over rows or over the batch (GroupNorm / LayerNorm parameter gradients, column sums, the gradient norm) has one
// launcher and two forms: float / double atomics (the f32 step), or a fixed summation order through a workspace (the 16-bit step,
// which is bitwise reproducible).  The workspace argument selects the form: null = atomics.
#pragma once
#include "t2p_common.h"

namespace t2p {

// ---- strided batched GEMM, fp32:  C[z][m][n] = alpha * sum_k A(z, m, k) B(z, k, n) + bias_n[n] + beta * C[z][m][n] ----------------
// A(z, m, k) = A[z0 sAz0 + z1 sAz1 + m sAm + k sAk], B(z, k, n) = B[z0 sBz0 + z1 sBz1 + k sBk + n sBn]: one of the two strides of
// an operand must be 1 (row- or column-major view), which covers x W^T, dY W, dY^T X, q k^T per head, P v, P^T dO ... without a
// transposed copy.  ksplit > 1 cuts the K loop over workgroups which add their partial tiles with hardware fp32 atomics (weight
// gradients: K = every pixel of the batch); it requires beta == 1 (accumulate into an initialised C).  ksplit == 0: chosen here.
struct TGemmArgs {
  const float* A = nullptr; long sAm = 0, sAk = 0, sAz0 = 0, sAz1 = 0;
  const float* B = nullptr; long sBk = 0, sBn = 0, sBz0 = 0, sBz1 = 0;
  float* C = nullptr; long ldc = 0, sCz0 = 0, sCz1 = 0;
  int M = 0, N = 0, K = 0, nz0 = 1, nz1 = 1;
  float alpha = 1.f, beta = 0.f;
  const float* bias_n = nullptr;
  int ksplit = 1;
  // weight gradient of a 3x3 convolution (layers.py:89-95): B is gathered, B(k = output pixel r, n = tap * conv_C + c) =
  // X[pixel(r) + offset(tap)][c] (zero outside the H x W map), X = [batch H W][ldx]; K = batch H W, N = 9 conv_C
  int conv_b = 0, H = 0, W = 0, conv_C = 0; long ldx = 0;
};
int launch_tgemm(const TGemmArgs& a, hipStream_t s);
// the same product on the 16-bit matrix pipe (mixed-precision training step): A and B stay fp32 in memory and are rounded to dtype
// (DT_F16 / DT_BF16, round to nearest even, no saturation) on the way into LDS; fp32 accumulation and epilogue.  Split-K (ksplit > 1,
// or chosen when ksplit == 0) writes partial tiles to ws and a second pass sums them in a fixed order: bitwise reproducible, any beta.
// ws: tgemm16_ws_floats(a) floats (0: no workspace needed)
long tgemm16_ws_floats(const TGemmArgs& a);
int launch_tgemm16(const TGemmArgs& a, int dtype, float* ws, hipStream_t s);

// ---- GroupNorm backward (nn.GroupNorm + optional SiLU, layers.py:282,304,317; attention.py:77) -------------------------------------
// y = act(gamma (x - mean) rstd + beta); x, dy, dx: NHWC [B][HW][C] fp32; stats [B][G][2] = (mean, rstd) of the forward pass.
// dx += ..., dgamma += ..., dbeta += ...;  ws: gn_bwd_ws_floats(B, HW, C, G) floats (both forms).  fixed_order: d gamma / d beta are
// summed over the batch in sample order instead of with atomics
long gn_bwd_ws_floats(int B, int HW, int C, int G);
int launch_gn_backward(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta, int silu,
                       int B, int HW, int C, int G, float* dx, float* dgamma, float* dbeta, float* ws, bool fixed_order, hipStream_t s);
// ---- LayerNorm backward (attention.py:203-205), rows x C, eps as the forward -----------------------------------------------------
// ws == nullptr: d gamma / d beta with atomics (C <= 8192); else fixed order, ws: ln_bwd_ws_floats(rows, C) floats
long ln_bwd_ws_floats(long rows, int C);
int launch_ln_backward(const float* x, const float* dy, const float* gamma, long rows, int C, float eps, float* dx, float* dgamma,
                       float* dbeta, float* ws, hipStream_t s);
// ---- softmax backward, in place: dP[r][j] <- scale P[r][j] (dP[r][j] - sum_j dP[r][j] P[r][j])  (P = softmax(scale S)) ------------------
int launch_softmax_backward(const float* P, float* dP, long rows, int n, float scale, hipStream_t s);
// ---- GEGLU backward (attention.py:37-44): u = [a | g], out = a gelu(g);  du += [dy gelu(g) | dy a gelu'(g)] ----------------------------
int launch_geglu_backward(const float* u, const float* dy, float* du, long rows, int inner, hipStream_t s);
// ---- elementwise ---------------------------------------------------------------------------------------------------------------------
int launch_silu(const float* x, float* y, long n, hipStream_t s);                                   // y = x sigmoid(x)
int launch_silu_backward(const float* x, const float* dy, float* dx, long n, hipStream_t s);        // dx += dy silu'(x)
int launch_axpy(float* y, const float* x, float a, long n, hipStream_t s);                          // y += a x
int launch_add_scale(const float* a, const float* b, float alpha, float* out, long n, hipStream_t s);   // out = alpha (a + b)
// dst[r][dst_off + c] (+)= src[r][src_off + c], c < C  (channel concat of the U-Net skips, ncsnpp.py:250, and its backward)
int launch_copy_cols(const float* src, long ld_src, long src_off, float* dst, long ld_dst, long dst_off, long rows, int C, int accumulate,
                     hipStream_t s);
// column sums: out[z][n] (+)= sum_r dy[z rows_per_z + r][n], dy rows of ld floats, out rows of ld_out.  nz = 1: bias gradients; nz = B:
// the gradient of the per-sample time-embedding bias (layers.py:316).  ws == nullptr: atomics; else fixed order, ws:
// colsum_ws_floats(nz, rows_per_z, N) floats
long colsum_ws_floats(int nz, long rows_per_z, int N);
int launch_colsum(const float* dy, int nz, long rows_per_z, int N, long ld, float* out, long ld_out, int accumulate, float* ws, hipStream_t s);
// nearest 2x up-sampling / 2x2 mean down-sampling of NHWC maps (layers.py:179-188) and their backward (+=)
int launch_up2(const float* x, float* y, int B, int H, int W, int C, hipStream_t s);               // x [B][H][W][C] -> y [B][2H][2W][C]
int launch_up2_backward(const float* dy, float* dx, int B, int H, int W, int C, hipStream_t s);
int launch_down2(const float* x, float* y, int B, int H, int W, int C, hipStream_t s);             // x [B][H][W][C] -> y [B][H/2][W/2][C]
int launch_down2_backward(const float* dy, float* dx, int B, int H, int W, int C, hipStream_t s);
// Dropout_0 (layers.py:318) with a given keep-mask (uint8, same layout as x): y = x keep / (1 - p);  backward dx += dy keep / (1 - p)
int launch_dropout(const float* x, const unsigned char* keep, float inv_keep, float* y, long n, int accumulate, hipStream_t s);
// keep-masks on the device: Philox4x32-10 keyed by (seed, stream id), element i kept iff its uniform >= p
int launch_dropout_mask(unsigned char* keep, long n, float p, unsigned long long seed, unsigned long long stream_id, hipStream_t s);

// ---- convolution weights between the reference layout and the kernels' layouts ----------------------------------------------------------
// w [Co][Ci][3][3] (nn.Conv2d) -> wf [Co][9][Cip] (forward implicit GEMM: K index = tap Cip + ci) and
//                                 wd [Ci][9][Cop] (input gradient = the same kernel on dY: wd[ci][t][co] = w[co][ci][8 - t]); pads are zero
int launch_conv_w_prep(const float* w, float* wf, float* wd, int Co, int Ci, int Cip, int Cop, hipStream_t s);
// gw [Co][Ci][3][3] += dwc [Co][9][Cip]
int launch_conv_w_grad_fold(const float* dwc, float* gw, int Co, int Ci, int Cip, hipStream_t s);

// ---- denoising score matching (losses.py:105-131) under the VE, VP and sub-VP SDEs -----------------------------------------------------
// VE, per sample: t[b] (given, or drawn here: t = eps + (T - eps) u, u from Philox keyed by (seed, step) -- losses.py:106 with T = 1),
// std[b] = sigma_min (sigma_max / sigma_min)^t (VESDE.marginal_prob, sde_lib.py:225-228), label[b] = round((1 - t) (N - 1)) (half to even:
// get_score_fn's VE branch, models/utils.py:165-168) and scale[b] = scale_by_sigma ? 1 / sigmas[label] : 1 (ncsnpp.py:256-261)
int launch_dsm_prepare(const float* t_in, int B, float t_eps, float sigma_min, float sigma_max, int N, const float* inv_sigma_table,
                       unsigned long long seed, unsigned long long step, float* t_out, float* std, int* labels, float* scale, hipStream_t s);
// VP (subvp = 0) / sub-VP (subvp = 1), per sample, t as above (the same Philox stream): lmc = -t^2 (beta_max - beta_min) / 4 - t beta_min / 2,
// mean_coef[b] = exp(lmc), std[b] = sqrt(1 - exp(2 lmc)) (VP, sde_lib.py:134-138) / 1 - exp(2 lmc) (sub-VP, sde_lib.py:184-188) with
// 1 - exp(2 lmc) = -expm1(2 lmc) in double; labels_f[b] = t (N - 1) (VP) / 999 t (sub-VP), the float the network embeds
// (models/utils.py:147,152); labels[b] = trunc(labels_f) (the sigma index, ncsnpp.py:223); scale[b] = -1 / std_table[labels[b]] (VP: the
// DISCRETE sqrt_1m_alphas_cumprod entry, models/utils.py:154) / -1 / std[b] (sub-VP, :149), times inv_sigma_table[labels[b]] when given.
// std_table: device float[N], VP only.  sub-VP with inv_sigma_table needs N >= 1000
int launch_dsm_prepare_vp(const float* t_in, int B, float t_eps, double beta_min, double beta_max, int subvp, int N, const float* std_table,
                          const float* inv_sigma_table, unsigned long long seed, unsigned long long step, float* t_out, float* mean_coef,
                          float* std, int* labels, float* labels_f, float* scale, hipStream_t s);
// mask[b][c][y][x] = mask_pair[b][y][x] && conditional_mask (length: c != C - 1; ss: c not in 4..6; inpainting: mask_inpaint[b][y][x]);
// perturbed = mask ? mean_coef[b] x + std[b] z : x (mean_coef == nullptr: the VE form x + std[b] z);  num_elem[b] = #mask
// (all NCHW; cond_flags: 1 length, 2 ss, 4 inpainting)
// ss_rows (optional, [B][L] from launch_ss_block_rows): block_dropout (losses.py:54-64) on the way in -- for c in 4..6 the x that enters
// BOTH branches of the select is 0 where ss_rows[b][y] | ss_rows[b][x].  The reference zeroes its coords_6d argument in place; here x
// itself is never written, the zeroing happens on the way into `perturbed`.  Without ss_rows: the kernels of a pass without blocks
int launch_dsm_perturb(const float* x, const float* z, const float* std, const float* mean_coef, const unsigned char* mask_pair,
                       const unsigned char* mask_inpaint, int cond_flags, int B, int C, int L, float* perturbed, unsigned char* mask,
                       float* num_elem, hipStream_t s, const unsigned char* ss_rows = nullptr);
// secondary-structure block list -> residue flags: rows [B][L] uint8 = 1 where residue r lies in a DROPPED block (zeroed here first).
// blocks: device int32 [n][3] = (sample, start, end), end exclusive, Python slice semantics on an axis of length L (end clamped to L,
// start >= end empty, overlaps fine; a negative index or a sample outside [0, B) writes nothing -- the host callers refuse them).
// drop: device uint8 [n] explicit decisions, or nullptr = drawn here: block k is dropped iff u < p, u = (c0 >> 8) 2^-24 of Philox4x32-10
// with counter k, stream id stream_id and key seed (the uniform of dsm_prepare's t).  drop_out (optional, [n]): the decisions used
int launch_ss_block_rows(const int* blocks, int n, const unsigned char* drop, float p, unsigned long long seed, unsigned long long stream_id,
                         int B, int L, unsigned char* rows, unsigned char* drop_out, hipStream_t s);
// text-context dropout, the decisions: drop [B] uint8 = 1 where sample b is dropped, iff u < p with u = (c0 >> 8) 2^-24 of Philox4x32-10,
// training layout, counter b, stream id stream_id, key seed (the uniform of dsm_prepare's t and of the block decisions)
int launch_context_drop_draw(int B, float p, unsigned long long seed, unsigned long long stream_id, unsigned char* drop, hipStream_t s);
// x0 and (optional) x1: fp32 [B][n], 16-byte aligned, n % 4 == 0.  Row b of each becomes +0.0f where drop[b] != 0 (stored, not multiplied:
// an Inf or a NaN becomes 0); the rows of the other samples are neither read nor written.  One launch for both buffers
int launch_zero_sample_rows(float* x0, float* x1, int B, long n, const unsigned char* drop, hipStream_t s);
// random_mask_batch (utils.py:15-60) drawn on the device: flags [B][L] uint8 (1 = residue masked) and pair [B][L][L] uint8 =
// flags[b][i] | flags[b][j], one workgroup per sample.  llh: device int32 [B][3] = (l, lo, hi), l valid residues, lo = int(min l),
// hi = int(max l) from the host; the callers guarantee 0 <= lo < hi <= l <= L <= 256.  mode: force_mode when >= 0, else drawn from one
// uniform u0: 1 (random subset) when u0 < p_random, 2 (contiguous window) when u0 > contig_above, else 0 (none: flags = 1 for all L,
// the padding included).  Counter indices within stream_id (training layout, key seed): philox.h's table.  Per sample
// r = lo + (((w0 >> 8) (hi - lo)) >> 24) residues are masked: the window start .. start + r with start = ((w1 >> 8) (l - r)) >> 24, or
// the r residues whose 32-bit keys rank lowest among the l (ties to the lower index).  mode_out (optional): device int, the mode used
int launch_inpaint_mask_draw(const int* llh, int B, int L, float p_random, float contig_above, unsigned long long seed,
                             unsigned long long stream_id, int force_mode, unsigned char* flags, unsigned char* pair, int* mode_out,
                             hipStream_t s);
// o: the head convolution's output NHWC [B][L L][ldo]; scale[b]: the signed per-sample output scale of dsm_prepare; score = scale[b] o;
// r = score std[b] + z; loss_sum[b] += sum mask r^2 (double);  d_o [B][L L][ld_do] = 2 r mask std scale / ((num_elem + 1e-8) B), pad columns zero
int launch_dsm_loss(const float* o, long ldo, const float* z, const float* std, const float* scale, const unsigned char* mask,
                    const float* num_elem, int B, int C, int L, double* loss_sum, float* d_o, long ld_do, float* score_nchw, hipStream_t s);
// loss = mean_b loss_sum[b] / (num_elem[b] + 1e-8)
int launch_dsm_finish(const double* loss_sum, const float* num_elem, int B, float* loss, hipStream_t s);

// ---- the DDIM sampler's noise-prediction objective (sampler/diffusion_sampler.py:144-167: q_sample, p_loss, forward) ----------------------
// per sample: the integer timestep t_b -- t_in[b] when given (fp32 holding an integer; clamped to [0, T - 1], NaN -> 0), else drawn:
// t_b = ((w >> 8) T) >> 24 with w = word 0 of Philox4x32-10, training layout, counter b, stream id stream_id, key seed (T <= 2^24) --
// then t_out[b] = labels[b] = t_b, mean_coef[b] = sqrt_ac[t_b], std[b] = sqrt_1mac[t_b] (device float[T] each): what
// launch_dsm_perturb's mean-coefficient path and launch_timestep_embedding's integer-label path take; scale[b] = inv_sigma_table[t_b]
// (device float[N], needs T <= N: UNetModel.forward's own division by sigmas[t], ncsnpp.py:259-261) or 1 without a table
int launch_ploss_prepare(const float* t_in, int B, int T, const float* sqrt_ac, const float* sqrt_1mac, const float* inv_sigma_table, int N,
                         unsigned long long seed, unsigned long long stream_id, float* t_out, float* mean_coef, float* std, int* labels,
                         float* scale, hipStream_t s);
// the draw alone, through the same device function: out [B] int32
int launch_ploss_draw_t(int B, int T, unsigned long long seed, unsigned long long stream_id, int* out, hipStream_t s);
// o: the head convolution's output NHWC [B][L L][ldo]; pred = scale[b] o, the predicted noise; r = pred - z; loss_sum[b] += sum mask |r|
// (l1) or mask r^2 (double); d_o [B][L L][ld_do] = mask sign(r) (sign(0) = 0) or mask 2 r, times scale[b] / ((num_elem + 1e-8) B), pad
// columns zero; pred_nchw (optional) = pred
int launch_ploss_loss(int l1, const float* o, long ldo, const float* z, const float* scale, const unsigned char* mask, const float* num_elem,
                      int B, int C, int L, double* loss_sum, float* d_o, long ld_do, float* pred_nchw, hipStream_t s);

// ---- optimizer (losses.py:26-51: Adam, warm-up, clip_grad_norm_) and EMA (ema.py:32-49) over flat parameter buffers ------------------------
// partial == nullptr: *out += sum g^2 with atomics (zero it first); else *out = sum g^2 in a fixed order, partial: 1024 doubles
int launch_sumsq(const float* g, long n, double* partial, double* out, hipStream_t s);
struct AdamArgs {
  float* p = nullptr; float* g = nullptr; float* m = nullptr; float* v = nullptr; long n = 0;
  float lr = 0.f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, weight_decay = 0.f;
  float one_minus_beta1 = 0.1f, one_minus_beta2 = 0.001f;   // rounded from double, as torch rounds its scalars: 1.f - 0.999f is 1.3e-5 off 0.001f
  float bias1 = 1.f, bias2_sqrt = 1.f;    // 1 - beta1^k, sqrt(1 - beta2^k)
  float grad_clip = -1.f;                 // >= 0: g *= min(1, grad_clip / (sqrt(*sumsq) + 1e-6)) first (written back, as clip_grad_norm_ does)
  const double* sumsq = nullptr;
};
int launch_adam(const AdamArgs& a, hipStream_t s);
int launch_ema(float* shadow, const float* p, float one_minus_decay, long n, hipStream_t s);   // shadow -= (1 - d) (shadow - p)
int launch_scale(float* x, float a, long n, hipStream_t s);                                   // x *= a
// s2[0] = S = 2^e, e = the largest integer with 2^e max|x| <= target, clamped to [-60, 60] (S and 1 / S stay normal floats for any
// maximum, a subnormal one included; beyond the clamp S max|x| <= target no longer holds); S = 1 when x is all zero or not finite;
// s2[1] = 1 / S; absmax: one device word of scratch.  The maximum is taken with integer atomics on the bit patterns: the same S whatever the order of arrival
int launch_seed_scale(const float* x, long n, float target, unsigned int* absmax, float* s2, hipStream_t s);
int launch_scale_dev(float* x, const float* a, long n, hipStream_t s);                        // x *= *a (a on the device)

}  // namespace t2p
