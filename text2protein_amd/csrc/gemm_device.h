// Device helpers and cross-unit declarations shared by the GEMM units: gemm.hip, gemm_dma.hip, gemm_splitk.hip, thin_conv.hip
// (the map of those files: top of gemm.hip).
#pragma once
#include "t2p_common.h"
#include "gemm_mfma.h"

namespace t2p {

typedef float f32x16 __attribute__((ext_vector_type(16)));

[[maybe_unused]] static constexpr int ROWB = 144;  // LDS row stride in bytes: 128 data + 16 pad

template <typename TC> struct VecInfo { static constexpr int VEC = 16 / (int)sizeof(TC); };

// pack VEC floats into 16 bytes of TC
template <typename TC> __device__ inline uint4 pack16(const float* f);
template <> __device__ inline uint4 pack16<float>(const float* f) {
  uint4 r;
  r.x = __builtin_bit_cast(uint32_t, f[0]); r.y = __builtin_bit_cast(uint32_t, f[1]);
  r.z = __builtin_bit_cast(uint32_t, f[2]); r.w = __builtin_bit_cast(uint32_t, f[3]);
  return r;
}
template <> __device__ inline uint4 pack16<bf16_t>(const float* f) {
  uint4 r;
  r.x = (uint32_t)f32_to_bf16_bits(f[0]) | ((uint32_t)f32_to_bf16_bits(f[1]) << 16);
  r.y = (uint32_t)f32_to_bf16_bits(f[2]) | ((uint32_t)f32_to_bf16_bits(f[3]) << 16);
  r.z = (uint32_t)f32_to_bf16_bits(f[4]) | ((uint32_t)f32_to_bf16_bits(f[5]) << 16);
  r.w = (uint32_t)f32_to_bf16_bits(f[6]) | ((uint32_t)f32_to_bf16_bits(f[7]) << 16);
  return r;
}
template <> __device__ inline uint4 pack16<f16_t>(const float* f) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  uint4 r;
  h2 a = {(_Float16)f[0], (_Float16)f[1]}, b = {(_Float16)f[2], (_Float16)f[3]};
  h2 c = {(_Float16)f[4], (_Float16)f[5]}, d = {(_Float16)f[6], (_Float16)f[7]};
  r.x = __builtin_bit_cast(uint32_t, a); r.y = __builtin_bit_cast(uint32_t, b);
  r.z = __builtin_bit_cast(uint32_t, c); r.w = __builtin_bit_cast(uint32_t, d);
  return r;
}

// zero the elements >= nvalid of a packed vector
template <typename TC> __device__ inline uint4 mask_tail(uint4 v, int nvalid) {
  constexpr int VEC = VecInfo<TC>::VEC;
  union { uint4 u; TC e[VEC]; } x;
  x.u = v;
#pragma unroll
  for (int i = 0; i < VEC; ++i)
    if (i >= nvalid) x.e[i] = from_f32<TC>(0.f);
  return x.u;
}

// load one staging vector (VEC K-elements) from a source row; `off` in elements
template <typename TC, bool SRC_F32>
__device__ inline uint4 load_vec(const void* base, long off) {
  constexpr int VEC = VecInfo<TC>::VEC;
  if constexpr (SRC_F32) {
    const float* p = (const float*)base + off;
    float f[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      float4 t = *(const float4*)(p + i);
      f[i] = t.x; f[i + 1] = t.y; f[i + 2] = t.z; f[i + 3] = t.w;
    }
    return pack16<TC>(f);
  } else {
    return *(const uint4*)((const TC*)base + off);
  }
}

template <typename TC> struct Mma;
template <> struct Mma<float> {
  __device__ static inline void run(const uint4& a, const uint4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, a.y), __builtin_bit_cast(float, b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, a.z), __builtin_bit_cast(float, b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, a.w), __builtin_bit_cast(float, b.w), c, 0, 0, 0);
  }
};
template <> struct Mma<bf16_t> {
  __device__ static inline void run(const uint4& a, const uint4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
};
template <> struct Mma<f16_t> {
  __device__ static inline void run(const uint4& a, const uint4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};

// residual operand: fp32, or the compute dtype when GemmParams::r_lowp (element index, not bytes)
template <typename TC> __device__ inline float res_load1(const float* R, long idx, int lowp) {
  if constexpr (sizeof(TC) == 2) { if (lowp) return to_f32(((const TC*)R)[idx]); }
  return R[idx];
}
template <typename TC> __device__ inline float4 res_load4(const float* R, long idx, int lowp) {
  if constexpr (sizeof(TC) == 2) {
    if (lowp) {
      const f32x4_res_t v = unpack4<TC>(*(const u32x2_res_t*)((const TC*)R + idx));
      return make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  return *(const float4*)(R + idx);
}

// true when reg_epilogue covers the launch (else the LDS-staged dma_epilogue runs; both give the same values)
__host__ __device__ __forceinline__ bool reg_epilogue_ok(const GemmParams& p, const int nsplit, const int dbg) {
  if (dbg & 4096) return false;
  const long c_cols = p.geglu ? p.N / 2 : p.N;
  const long c_bytes = nsplit > 1 ? (long)p.M * p.N * 4 : ((long)(p.M - 1) * p.ldc + c_cols) * (p.c_f32 ? 4 : 2);
  const int HW = p.H * p.W;
  const long r_rows = p.r_up ? (long)(p.M / HW) * (p.H >> 1) * (p.W >> 1) : (long)p.M;
  const long r_bytes = p.R ? ((r_rows - 1) * p.ldr + p.N) * (p.r_lowp ? 2 : 4) : 0;
  if ((p.N & 7) || c_bytes >= (1L << 31) || r_bytes >= (1L << 31)) return false;
  if (nsplit > 1) return true;                                   // raw fp32 partial tiles [M][N]
  if (p.geglu ? (p.ldc & 3) : (p.ldc & 7)) return false;         // 16-byte aligned row segments (8 bytes for GEGLU's half-width rows)
  if (p.R && (p.ldr & 7)) return false;
  if (p.bias_bn && ((p.ld_bn & 3) || p.rows_per_batch % 16)) return false;
  if (p.r_up && (p.W % 16 || p.rows_per_batch != HW)) return false;
  return true;
}

struct DmaPlan { int geom, nsplit; };
// gemm.hip
int num_cus();
DmaPlan dma_plan(const GemmParams& p);
// gemm_dma.hip: instantiated for (f16_t, bf16_t) x (MODE 0, 1, 2)
template <typename TC, int MODE> int launch_dma_mode(const GemmParams& p, hipStream_t stream);
// gemm_splitk.hip
bool splitk_reduce_vec_ok(const GemmParams& p);
int launch_splitk_reduce(const GemmParams& p, int nsplit, hipStream_t stream);
// thin_conv.hip
int launch_thin_conv(const GemmParams& p, hipStream_t stream);

}  // namespace t2p
