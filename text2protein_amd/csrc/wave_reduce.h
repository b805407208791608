// Fixed-order reductions over a wavefront and over a workgroup: the one place they are written.
//
// A butterfly over the lanes with offsets 32, 16, ..., 1 leaves the same bits in every lane; a workgroup reduction then adds the
// wavefronts' values in wave order.  Nothing here depends on which lane or wavefront arrives first, so two calls give the same bits --
// the contract every structure operator and every training reduction states in its file head.
#pragma once
#include <hip/hip_runtime.h>

namespace t2p {

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// sums over aligned groups of LANES lanes (a power of two below 64), in place: offsets LANES / 2, ..., 1, every value at each offset
template <int LANES, typename... T> __device__ __forceinline__ void lanes_sum(T&... v) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1) ((v += __shfl_xor(v, off, 64)), ...);
}

// sums of NV values over a workgroup of NW wavefronts, the same bits in every thread; `red` holds NW * NV values
template <int NV, int NW, typename T> __device__ __forceinline__ void block_sum(T (&v)[NV], T* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if (lane == 0)
    for (int k = 0; k < NV; ++k) red[w * NV + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    T s = 0;
    for (int q = 0; q < NW; ++q) s += red[q * NV + k];
    v[k] = s;
  }
}
// maximum over a workgroup of NW wavefronts, the same bits in every thread; `red` holds NW doubles
template <int NW> __device__ __forceinline__ double block_max(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_max(v);
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  for (int q = 0; q < NW; ++q) v = fmax(v, red[q]);
  return v;
}

}  // namespace t2p
