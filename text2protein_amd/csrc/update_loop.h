// The element-wise tail every sampler shares: one thread per quad of consecutive elements (the unit of a Philox draw) forms the
// score s = scale (w o_c + w1 o_u), applies an update functor, re-masks and stores.  The Langevin and predictor updates (kernels.hip)
// and the DDIM update (ddim.hip) are instantiations.  Device code: include from .hip sources only.
#pragma once
#include <initializer_list>

#include "philox.h"
#include "t2p_kernels.h"

namespace t2p {

// Each product and sum of the guidance sum rounds to float32 in this order (reference sampler/diffusion_sampler.py:128); the scale
// (1 for VE and DDIM, -1 / std for VP) multiplies the rounded sum.  o_u absent: s = fl(scale o_c), and scale == 1 is exact.
__device__ inline float guided_score(float oc, float ou, bool guided, float w, float w1, float scale) {
#pragma clang fp contract(off)
  float o = oc;
  if (guided) {
    const float pc = w * oc, pu = w1 * ou;
    o = pc + pu;
  }
  return o * scale;
}
// a b + c d with both products rounded
__device__ inline float sum_of_products(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float ab = a * b, cd = c * d;
  return ab + cd;
}
// r = fl(fl(a d) + fl(z s)) of the replacement (inpainting.py:43-44); *mean = fl(a d)
__device__ inline float noised_data(float a, float d, float z, float s, float* mean) {
#pragma clang fp contract(off)
  const float ad = a * d, zs = z * s;
  *mean = ad;
  return ad + zs;
}
__device__ inline float guided_scale(const GuidedScore& g) {
  return g.scale_table ? g.scale_table[min(max(*g.step_counter, 0), g.n_table - 1)] : g.scale;
}

// the 16-byte path of the quad kernels: n % 4 == 0 and every pointer 16-byte aligned (the mask 4-byte); null counts as aligned
static inline bool quad_vec_ok(long n, std::initializer_list<const void*> p16, const void* mask) {
  bool ok = n % 4 == 0 && ((uintptr_t)mask % 4) == 0;
  for (const void* p : p16) ok = ok && ((uintptr_t)p % 16) == 0;
  return ok;
}

// Where z comes from: a.noise when given; else, with DRAW and `on`, the draw of t2p_op_philox_normal(seed, stream_id) for the quad
// (step word 0); else zeros.  Kernels instantiated without DRAW carry no generator.
struct QuadDraw {
  bool on = false;
  unsigned long long seed = 0, stream_id = 0;
};

// loads, s per element, UPDATE(x, s, z, &second) -> x_next, the mask, the stores: x_next to a.x_out and x_out2 (optional: the other
// half of the [x ; x] input of a guided evaluation), `second` (x_mean / the clean-sample prediction, never masked) to a.x_mean_out.
// VEC: quad_vec_ok holds and a quad moves as one 16-byte access per tensor; otherwise element by element, bounded by a.n.
// REPL: the replacement branch (InpaintReplace, r.known set): per element, frozen by the mask -> x_initial; else known -> the noised
// data; else the update.  `second` becomes fl(a d) where replaced and x_next elsewhere (inpainting.py:46).  The second normal is
// drawn here (nobody else reads it) unless r.noise gives it; a quad without a known element draws nothing.
template <bool VEC, bool DRAW, bool REPL = false, typename Update>
__device__ inline void update_loop(const SdeUpdateArgs& a, const GuidedScore& g, float* x_out2, const QuadDraw& d, Update update,
                                   const InpaintReplace& r = InpaintReplace()) {
  const float scale = guided_scale(g);
  float ra = 1.f, rs = 0.f;
  uint32_t rstep = 0u;
  if (REPL) {
    const int st = r.step_counter ? *r.step_counter : (int)r.step;
    rstep = (uint32_t)st;
    ra = r.mean_table ? r.mean_table[min(max(st, 0), r.n_table - 1)] : r.mean_coef;
    rs = r.std_table ? r.std_table[min(max(st, 0), r.n_table - 1)] : r.std;
  }
  const long nq = (a.n + 3) / 4;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
    const long i = q * 4;
    const int cnt = VEC ? 4 : (int)(a.n - i < 4 ? a.n - i : 4);
    alignas(16) float x[4], c[4], u[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f}, xi[4] = {0.f, 0.f, 0.f, 0.f};
    alignas(4) unsigned char m[4] = {1, 1, 1, 1};
    alignas(16) float dd[4] = {0.f, 0.f, 0.f, 0.f}, rz[4] = {0.f, 0.f, 0.f, 0.f};
    alignas(4) unsigned char kn[4] = {0, 0, 0, 0};
    if (VEC) {
      *(float4*)x = *(const float4*)(a.x + i);
      *(float4*)c = *(const float4*)(g.o_c + i);
      if (g.o_u) *(float4*)u = *(const float4*)(g.o_u + i);
      if (a.noise) *(float4*)z = *(const float4*)(a.noise + i);
      if (a.mask) {
        *(uchar4*)m = *(const uchar4*)(a.mask + i);
        *(float4*)xi = *(const float4*)(a.x_initial + i);
      }
      if (REPL) {
        *(uchar4*)kn = *(const uchar4*)(r.known + i);
        *(float4*)dd = *(const float4*)(r.data + i);
        if (r.noise) *(float4*)rz = *(const float4*)(r.noise + i);
      }
    } else {
      for (int k = 0; k < 4; ++k) x[k] = c[k] = 0.f;
      for (int k = 0; k < cnt; ++k) {
        x[k] = a.x[i + k];
        c[k] = g.o_c[i + k];
        if (g.o_u) u[k] = g.o_u[i + k];
        if (a.noise) z[k] = a.noise[i + k];
        if (a.mask) { m[k] = a.mask[i + k]; xi[k] = a.x_initial[i + k]; }
        if (REPL) {
          kn[k] = r.known[i + k];
          dd[k] = r.data[i + k];
          if (r.noise) rz[k] = r.noise[i + k];
        }
      }
    }
    if (DRAW && d.on) {
      uint32_t ctr[4];
      philox_counter_sampling(ctr, q, d.stream_id, 0u);
      philox4x32_10(ctr, d.seed);
      philox_normal4(ctr, z);
    }
    alignas(16) float xn[4], xm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xn[k] = update(x[k], guided_score(c[k], u[k], g.o_u != nullptr, g.w, g.w1, scale), z[k], &xm[k]);
      if (!m[k]) xn[k] = xi[k];
    }
    if (REPL) {
      if (!r.noise && (kn[0] | kn[1] | kn[2] | kn[3])) {
        uint32_t ctr[4];
        philox_counter_sampling(ctr, q, r.stream, rstep);
        philox4x32_10(ctr, r.seed);
        philox_normal4(ctr, rz);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float ad;
        const float rr = noised_data(ra, dd[k], rz[k], rs, &ad);
        const bool rep = kn[k] && m[k];
        xn[k] = rep ? rr : xn[k];
        xm[k] = rep ? ad : xn[k];
      }
    }
    if (VEC) {
      *(float4*)(a.x_out + i) = *(const float4*)xn;
      if (x_out2) *(float4*)(x_out2 + i) = *(const float4*)xn;
      if (a.x_mean_out) *(float4*)(a.x_mean_out + i) = *(const float4*)xm;
    } else {
      for (int k = 0; k < cnt; ++k) {
        a.x_out[i + k] = xn[k];
        if (x_out2) x_out2[i + k] = xn[k];
        if (a.x_mean_out) a.x_mean_out[i + k] = xm[k];
      }
    }
  }
}

}  // namespace t2p
