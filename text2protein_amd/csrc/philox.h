// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants): the only statement of
// the generator on the device.  Stateless: every draw is a pure function of (key, counter).  The key is always the 64-bit seed,
// (seed lo, seed hi).  oracle/philox.py restates this file in numpy; tests/test_gpu_philox.py pins the drawn bits.
//
// Who draws what.  Two counter layouts exist and are kept apart (unifying them changes drawn bits):
//   sampling layout  {q lo, q hi, (uint32) stream, step}      q = index of a quad of consecutive elements; four normals per counter
//   training layout  {i lo, i hi, stream lo, stream hi}       i = quad / sample / block index; uniforms
//
//   drawer                                  key            layout    stream                       step word   counter   output
//   --------------------------------------  -------------  --------  ---------------------------  ----------  --------  ---------------------------
//   PC sampler (sampler.cpp)  prior         sampler seed   sampling  0                            0           quad q    normals (VE: x sigma_max)
//                             predictor     sampler seed   sampling  1                            loop step   quad q    normals
//                             corrector k   sampler seed   sampling  2 k + 2                      loop step   quad q    normals
//                             replace, after the corrector   sampler seed   sampling  0x80000000   loop step   quad q    normals, in the Langevin update kernel
//                             replace, after the predictor   sampler seed   sampling  0x80000001   loop step   quad q    normals, in the predictor update kernel
//                             (replacement inpainting, update_loop.h; disjoint from 0, 1 and 2 k + 2 for every k < 2^30 - 1)
//   DDIM (ddim.hip)           prior        sampler seed   sampling  0                            0           quad q    normals
//                             step i        sampler seed   sampling  i + 1                        0           quad q    normals, in the update kernel
//   t2p_op_philox_normal                    caller's seed  sampling  caller's                     0           quad q    normals
//   Trainer (train.h)         times t       trainer seed   training  rng_t()  = calls             -           sample b  word 0: t = eps + (1 - eps) u
//                             noise z       trainer seed   sampling  rng_z()  = 4096 calls + 1    0           quad q    normals
//                             ss blocks     trainer seed   training  rng_ss() = 4096 calls + 2    -           block k   word 0: dropped when u < p
//                             inpaint mask  trainer seed   training  rng_inpaint() = 4096 calls + 3  -        0         word 0: the mode (random / contiguous / none)
//                                                                                                               (b + 1) 2^32       sample b, word 0: r = lo + (((w >> 8) (hi - lo)) >> 24),
//                                                                                                                                  word 1: start = ((w >> 8) (l - r)) >> 24
//                                                                                                               (b + 1) 2^32 + 1 + j   word 0: the 32-bit key of residue j (the r lowest are masked)
//                             context drop  trainer seed   training  rng_ctx() = 4096 calls + 4   -           sample b  word 0: the text context dropped when u < p
//                             p_loss t      trainer seed   training  rng_ploss_t() = 4096 calls + 5  -        sample b  word 0: t = ((w >> 8) timesteps) >> 24 (set_ploss)
//                             Dropout_0 k   trainer seed   training  rng_dropout(k)            -           quad q    4 words: element 4 q + j kept
//                                                                      = 4096 calls + 16 + k                            when u_j >= p
//   t2p_op_inpaint_mask_draw                caller's seed  training  caller's                     -           as the trainer's inpaint mask
//   t2p_op_context_drop                     caller's seed  training  caller's                     -           as the trainer's context drop
//   t2p_op_ploss_draw_t                     caller's seed  training  caller's                     -           as the trainer's p_loss t
//   t2p_op_perturb_torsions                 caller's seed  training  caller's + candidate k       -           residue i + 2^32 chain_id   word 0: dphi_i, word 1: dpsi_i
//   (refine_rounds.hip)                                                                                                  = amp (2 u - 1) degrees
//   t2p_op_refine_rounds                    caller's seed  training  stream_base + 16 round + k   -           as t2p_op_perturb_torsions
//   (calls = Trainer::loss_calls_, the number of loss calls completed before the running one.)
//
// Two known defects, recorded here and left as they are (fixing either changes drawn bits):
//   * the sampling layout keeps only the low 32 bits of a stream id: streams s and s + 2^32 draw the same numbers (the trainer's z stream
//     wraps after 2^20 loss calls);
//   * rng_t() is `calls`, not `4096 calls`: from the 4097th loss call on it repeats (key, stream) pairs that earlier calls used for z, the
//     block decisions and the keep-masks (call 4096 n + 1 repeats z's stream of call n), under the other counter layout.
#pragma once
#include "t2p_common.h"

namespace t2p {

// the ten rounds on counter c under key (k0, k1), the key bumped by the Weyl constants between rounds
__device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__device__ inline void philox4x32_10(uint32_t (&c)[4], unsigned long long seed) { philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32)); }

// the two counter layouts of the table above
__device__ inline void philox_counter_sampling(uint32_t (&c)[4], long q, unsigned long long stream, uint32_t step) {
  c[0] = (uint32_t)q; c[1] = (uint32_t)((unsigned long long)q >> 32); c[2] = (uint32_t)stream; c[3] = step;
}
__device__ inline void philox_counter_training(uint32_t (&c)[4], long i, unsigned long long stream) {
  c[0] = (uint32_t)i; c[1] = (uint32_t)((unsigned long long)i >> 32); c[2] = (uint32_t)stream; c[3] = (uint32_t)(stream >> 32);
}

__device__ inline float philox_uniform24(uint32_t w) { return (w >> 8) * (1.0f / 16777216.0f); }     // [0, 1)

// Box-Muller on the word pairs (0, 1) -> z0, z1 and (2, 3) -> z2, z3, cosine first
__device__ inline void philox_normal4(const uint32_t (&c)[4], float (&z)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);   // (0, 1)
    const float u2 = (float)(c[2 * h + 1] >> 8) * (1.0f / 16777216.0f);         // [0, 1)
    const float rad = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = rad * cs;
    z[2 * h + 1] = rad * sn;
  }
}

}  // namespace t2p
