// Device helpers shared by the 16x16x32 MFMA kernels (gemm_dma.hip, thin_conv.hip, rowgemm.hip): fragment types, the MFMA wrapper, buffer
// descriptors, the channel permutation of a wave's 64-column block and the arithmetic of the register epilogue.
#pragma once
#include "t2p_common.h"

namespace t2p {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_res_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_res_t __attribute__((ext_vector_type(2)));
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
#define T2P_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
[[maybe_unused]] static constexpr unsigned DMA_OOB = 0x80000000u;   // >= any num_records we accept -> zeros

template <typename TC> __device__ inline f32x4_res_t unpack4(u32x2_res_t u) {     // four 16-bit values -> fp32
  TC e[4];
  e[0] = __builtin_bit_cast(TC, (uint16_t)u.x); e[1] = __builtin_bit_cast(TC, (uint16_t)(u.x >> 16));
  e[2] = __builtin_bit_cast(TC, (uint16_t)u.y); e[3] = __builtin_bit_cast(TC, (uint16_t)(u.y >> 16));
  return (f32x4_res_t){to_f32(e[0]), to_f32(e[1]), to_f32(e[2]), to_f32(e[3])};
}

// erf-GELU for the fused GEGLU epilogue (16-bit outputs only): Abramowitz-Stegun 7.1.26, |error| of
// erf <= 1.5e-7 -- far below the fp16 / bf16 rounding of the result -- in a dozen VALU operations
// instead of the branchy libm erff.
__device__ inline float gelu_erf_fast(float g) {
  const float x = g * 0.70710678118654752440f, ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
  float q = fmaf(t, 1.061405429f, -1.453152027f);
  q = fmaf(q, t, 1.421413741f);
  q = fmaf(q, t, -0.284496736f);
  q = fmaf(q, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-ax * ax * 1.44269504088896340736f);
  const float erf_abs = fmaf(-q * t, e, 1.f);
  return 0.5f * g * (1.f + copysignf(erf_abs, x));
}
// two fp32 values rounded to the compute dtype, packed low / high
template <typename TC> __device__ inline uint32_t pack2(float a, float b) {
  const TC x = from_f32<TC>(a), y = from_f32<TC>(b);
  return (uint32_t)__builtin_bit_cast(uint16_t, x) | ((uint32_t)__builtin_bit_cast(uint16_t, y) << 16);
}

template <typename TC> struct Mma16;
template <> struct Mma16<bf16_t> {
  __device__ static inline void run(const u32x4_t& a, const u32x4_t& b, f32x4_t& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
};
template <> struct Mma16<f16_t> {
  __device__ static inline void run(const u32x4_t& a, const u32x4_t& b, f32x4_t& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};
template <int I> __device__ inline void lds_read_b128_2k(u32x4_t& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(I * 2048));
}

// buffer descriptor covering `bytes` from `base`: everything beyond reads as zero / is dropped on store.  Built from
// readfirstlane'd scalars so that hipcc keeps it in SGPRs (no waterfall loop around the DMA).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int bytes) {
  const unsigned long long b = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  const int nb = __builtin_amdgcn_readfirstlane(bytes);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, nb, 0x00020000);
}

// The 16x16x32 kernels feed the WEIGHT fragment as the MFMA's first operand and permute the weight rows of a wave's 64-column
// block (see reg_epilogue in gemm_dma.hip): row rho (0..63) of the block as the MFMA sees it -> channel of the block
__host__ __device__ __forceinline__ int hperm(int rho) {
  const int j = rho >> 4, g = (rho >> 2) & 3, v = rho & 3;
  return 32 * (j >> 1) + 8 * g + 4 * (j & 1) + v;
}

}  // namespace t2p
