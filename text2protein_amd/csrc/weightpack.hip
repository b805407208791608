// Weight packing on the device: the re-layouts and weight products Engine::finalize performs on the host, as kernels that read slices
// of a flat fp32 parameter buffer (the trainer's parameters or EMA shadow) and write one of the engine's persistent weight buffers in
// the compute dtype.  Every kind produces the bits of its host twin (weight_pack_host, engine.cpp): the re-layouts move values, the
// conversions round to nearest even on both sides, and the two products repeat the host loop's arithmetic -- one fp32 accumulator from
// 0, terms in ascending k, a rounded product then a rounded add (the host library is built for the x86-64 baseline, which has no fma).
// hipcc contracts a * b + c into an fma by default -- also through __fmul_rn / __fadd_rn, which are inline operators carrying the
// header's contraction flags (the ISA of a first version held v_pk_fma_f32) -- so the pragma below switches contraction off for this
// whole file and the arithmetic is written with plain operators: every product and every sum here is rounded on its own.
//
// All kernels are bandwidth-bound (or tiny).  The transposing kinds stage a tile in LDS so that both the fp32 reads and the stores are
// contiguous runs: WP_CONV3 / WP_UP4 read the [channel][9] block of one output row whole and write each tap's channel run whole;
// WP_NIN moves 64 x 64 tiles, so a 16-bit store run is one 128-byte line.
#include <algorithm>

#include "t2p_kernels.h"

#pragma clang fp contract(off)

namespace t2p {
namespace {

constexpr int CT = 256;        // channels of one WP_CONV3 / WP_UP4 tile (9 KiB of LDS)
constexpr int NT = 64;         // WP_NIN tile edge
constexpr int PT = 32;         // WP_PRODUCT tile edge

inline int wp_grid(long n, int per_block = 256) { return (int)std::min<long>((n + per_block - 1) / per_block, 4096); }

// dst = src0[0:n0] | src1[0:n1] | src2[0:n2]
template <typename T>
__global__ __launch_bounds__(256) void wp_copy_kernel(const float* __restrict__ s0, long n0, const float* __restrict__ s1, long n1,
                                                      const float* __restrict__ s2, long n2, T* __restrict__ dst) {
  const long n = n0 + n1 + n2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = i < n0 ? s0[i] : (i < n0 + n1 ? s1[i - n0] : s2[i - n0 - n1]);
    dst[i] = from_f32<T>(v);
  }
}
// one source whose address, length and destination are 16-byte friendly: four values per lane
template <typename T>
__global__ __launch_bounds__(256) void wp_copy4_kernel(const float4* __restrict__ s0, long n4, T* __restrict__ dst) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = s0[i];
    alignas(16) T o[4] = {from_f32<T>(v.x), from_f32<T>(v.y), from_f32<T>(v.z), from_f32<T>(v.w)};
    if constexpr (sizeof(T) == 4) *reinterpret_cast<float4*>(dst + 4 * i) = *reinterpret_cast<const float4*>(o);
    else *reinterpret_cast<uint2*>(dst + 4 * i) = *reinterpret_cast<const uint2*>(o);
  }
}

// dst[r * ld + j] = src[r * rowlen + j]
template <typename T>
__global__ __launch_bounds__(256) void wp_rows_kernel(const float* __restrict__ src, long rows, long rowlen, long ld, T* __restrict__ dst) {
  const long n = rows * rowlen;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / rowlen, j = i - r * rowlen;
    dst[r * ld + j] = from_f32<T>(src[i]);
  }
}

// (N, Ci, 3, 3) -> dst[n * ld + tap * cp + c], channels Ci .. cp - 1 zero.  Block (x = channel tile, y = n)
template <typename T>
__global__ __launch_bounds__(256) void wp_conv3_kernel(const float* __restrict__ src, int Ci, int cp, long ld, T* __restrict__ dst) {
  __shared__ float tile[CT * 9];
  const int n = blockIdx.y, c0 = blockIdx.x * CT;
  const int nc = min(CT, Ci - c0);            // source channels of this tile (<= 0: padding only)
  const int nw = min(CT, cp - c0);            // destination channels
  const float* s = src + ((long)n * Ci + c0) * 9;
  for (int i = threadIdx.x; i < nc * 9; i += 256) tile[i] = s[i];
  __syncthreads();
  T* d = dst + (long)n * ld + c0;
  for (int tap = 0; tap < 9; ++tap)
    for (int c = threadIdx.x; c < nw; c += 256) d[(long)tap * cp + c] = from_f32<T>(c < nc ? tile[c * 9 + tap] : 0.f);
}

// conv0 of an up block as four 2 x 2 phase convolutions: dst[((ph * co + n) * 4 + tap) * ci + c] = the 3x3 taps that read the same
// source pixel, summed in fp32 in (kh, kw) order from 0, rounded once
__device__ inline int wp_fl2(int f) { return f >= 0 ? f / 2 : -((-f + 1) / 2); }
template <typename T>
__global__ __launch_bounds__(256) void wp_up4_kernel(const float* __restrict__ src, int co, int ci, T* __restrict__ dst) {
  __shared__ float tile[CT * 9];
  const int n = blockIdx.y, c0 = blockIdx.x * CT;
  const int nc = min(CT, ci - c0);
  const float* s = src + ((long)n * ci + c0) * 9;
  for (int i = threadIdx.x; i < nc * 9; i += 256) tile[i] = s[i];
  __syncthreads();
  for (int ph = 0; ph < 4; ++ph) {
    const int py = ph >> 1, px = ph & 1;
    for (int tap = 0; tap < 4; ++tap) {
      const int ty = tap >> 1, tx = tap & 1;
      T* d = dst + (((long)ph * co + n) * 4 + tap) * ci + c0;
      for (int c = threadIdx.x; c < nc; c += 256) {
        float acc = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw)
            if (wp_fl2(py + kh - 1) + 1 - py == ty && wp_fl2(px + kw - 1) + 1 - px == tx) acc = acc + tile[c * 9 + kh * 3 + kw];
        d[c] = from_f32<T>(acc);
      }
    }
  }
}

// (N, C, 3, 3) -> dst[(tap * C + c) * N + n] (the direct input convolution: lanes = output channels).  Block = 32 output channels
template <typename T>
__global__ __launch_bounds__(256) void wp_conv3_t_kernel(const float* __restrict__ src, int N, int C, T* __restrict__ dst) {
  extern __shared__ float dyn_tile[];
  const int K9 = C * 9, st = K9 | 1;          // odd row stride: the 32 rows of one store run sit in 32 different banks
  const int n0 = blockIdx.x * 32, nn = min(32, N - n0);
  const float* s = src + (long)n0 * K9;
  for (int i = threadIdx.x; i < nn * K9; i += 256) dyn_tile[(i / K9) * st + i % K9] = s[i];
  __syncthreads();
  const int j = threadIdx.x & 31;
  if (j >= nn) return;
  for (int k = threadIdx.x >> 5; k < K9; k += 8) {
    const int tap = k / C, c = k - tap * C;   // destination column k = tap * C + c reads source column c * 9 + tap
    dst[(long)k * N + n0 + j] = from_f32<T>(dyn_tile[j * st + c * 9 + tap]);
  }
}

// NIN (K, N) -> dst[z * N * K + n * K + k], z = which of up to two sources
template <typename T>
__global__ __launch_bounds__(256) void wp_nin_kernel(const float* __restrict__ s0, const float* __restrict__ s1, int K, int N, T* __restrict__ dst) {
  __shared__ float tile[NT][NT + 1];
  const float* src = blockIdx.z ? s1 : s0;
  T* d = dst + (long)blockIdx.z * N * K;
  const int n0 = blockIdx.x * NT, k0 = blockIdx.y * NT;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < NT; r += 4)
    if (k0 + r < K && n0 + tx < N) tile[r][tx] = src[(long)(k0 + r) * N + n0 + tx];
  __syncthreads();
  for (int r = ty; r < NT; r += 4)
    if (n0 + r < N && k0 + tx < K) d[(long)(n0 + r) * K + k0 + tx] = from_f32<T>(tile[tx][r]);
}

// GEGLU projection (2 * inner, rowlen): row 2 j = value_j (source row j), row 2 j + 1 = gate_j (source row inner + j)
template <typename T>
__global__ __launch_bounds__(256) void wp_geglu_kernel(const float* __restrict__ src, long inner, long rowlen, T* __restrict__ dst) {
  const long n = 2 * inner * rowlen;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / rowlen, j = i - r * rowlen;
    const long sr = (r >> 1) + ((r & 1) ? inner : 0);
    dst[i] = from_f32<T>(src[sr * rowlen + j]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void wp_add_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, T* __restrict__ dst) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = from_f32<T>(a[i] + b[i]);
}

// prod[m][n] = sum_k A[m][k] B[k][n] (+ addv[n]), the host loop's arithmetic; stored at dst[m * ld + n], or dst[n * ld + m] (transposed).
// 32 x 32 outputs per block, four rows per lane; the tile turns in LDS so that either orientation stores whole runs
template <typename T>
__global__ __launch_bounds__(256) void wp_product_kernel(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ addv,
                                                         int M, int K, int N, int transposed, long ld, T* __restrict__ dst) {
  __shared__ float tile[PT][PT + 1];
  const int n0 = blockIdx.x * PT, m0 = blockIdx.y * PT;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int n = n0 + tx;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* a[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = A + (long)min(m0 + ty + 8 * i, M - 1) * K;      // rows past M: computed, never stored
  if (n < N) {
    for (int k = 0; k < K; ++k) {
      const float b = B[(long)k * N + n];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float prod = a[i][k] * b;      // rounded here (contraction is off in this file) ...
        acc[i] = acc[i] + prod;              // ... and here
      }
    }
    if (addv) {
      const float v = addv[n];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = acc[i] + v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = acc[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + 8 * i;
    if (!transposed) {
      if (m0 + r < M && n0 + tx < N) dst[(long)(m0 + r) * ld + n0 + tx] = from_f32<T>(tile[r][tx]);
    } else {
      if (n0 + r < N && m0 + tx < M) dst[(long)(n0 + r) * ld + m0 + tx] = from_f32<T>(tile[tx][r]);
    }
  }
}

// dst[n] = (float)(b0[n] + sum_j (double)W[n][j] * v[j]): one double accumulator, ascending j, rounded product then rounded add
template <typename T>
__global__ __launch_bounds__(256) void wp_dot64_kernel(const float* __restrict__ W, const float* __restrict__ v, const float* __restrict__ b0,
                                                       int N, int K, T* __restrict__ dst) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double acc = (double)b0[n];
  const float* w = W + (long)n * K;
  for (int j = 0; j < K; ++j) {
    const double prod = (double)w[j] * (double)v[j];
    acc = acc + prod;
  }
  dst[n] = from_f32<T>((float)acc);
}

template <typename T>
int launch_typed(const WeightPack& p, hipStream_t s) {
  const int64_t* d = p.d;
  T* dst = (T*)p.dst;
  const float* const* src = p.src;
  switch (p.kind) {
    case WP_COPY: {
      const long n = d[0] + d[1] + d[2];
      const bool one = d[1] == 0 && d[2] == 0;
      if (one && n % 4 == 0 && ((uintptr_t)src[0] | (uintptr_t)dst) % 16 == 0)
        hipLaunchKernelGGL(wp_copy4_kernel<T>, dim3(wp_grid(n / 4)), dim3(256), 0, s, (const float4*)src[0], n / 4, dst);
      else
        hipLaunchKernelGGL(wp_copy_kernel<T>, dim3(wp_grid(n)), dim3(256), 0, s, src[0], (long)d[0], src[1], (long)d[1], src[2], (long)d[2], dst);
      break;
    }
    case WP_ROWS:
      hipLaunchKernelGGL(wp_rows_kernel<T>, dim3(wp_grid(d[0] * d[1])), dim3(256), 0, s, src[0], (long)d[0], (long)d[1], (long)d[2], dst);
      break;
    case WP_CONV3:
      hipLaunchKernelGGL(wp_conv3_kernel<T>, dim3((unsigned)((d[2] + CT - 1) / CT), (unsigned)d[0]), dim3(256), 0, s, src[0], (int)d[1], (int)d[2],
                         (long)d[3], dst);
      break;
    case WP_CONV3_T:
      hipLaunchKernelGGL(wp_conv3_t_kernel<T>, dim3((unsigned)((d[0] + 31) / 32)), dim3(256), (size_t)32 * ((d[1] * 9) | 1) * 4, s, src[0], (int)d[0],
                         (int)d[1], dst);
      break;
    case WP_NIN:
      hipLaunchKernelGGL(wp_nin_kernel<T>, dim3((unsigned)((d[1] + NT - 1) / NT), (unsigned)((d[0] + NT - 1) / NT), (unsigned)d[2]), dim3(256), 0, s,
                         src[0], src[1], (int)d[0], (int)d[1], dst);
      break;
    case WP_GEGLU:
      hipLaunchKernelGGL(wp_geglu_kernel<T>, dim3(wp_grid(2 * d[0] * d[1])), dim3(256), 0, s, src[0], (long)d[0], (long)d[1], dst);
      break;
    case WP_UP4:
      hipLaunchKernelGGL(wp_up4_kernel<T>, dim3((unsigned)((d[1] + CT - 1) / CT), (unsigned)d[0]), dim3(256), 0, s, src[0], (int)d[0], (int)d[1], dst);
      break;
    case WP_ADD:
      hipLaunchKernelGGL(wp_add_kernel<T>, dim3(wp_grid(d[0])), dim3(256), 0, s, src[0], src[1], (long)d[0], dst);
      break;
    case WP_PRODUCT:
      hipLaunchKernelGGL(wp_product_kernel<T>, dim3((unsigned)((d[2] + PT - 1) / PT), (unsigned)((d[0] + PT - 1) / PT)), dim3(256), 0, s, src[0], src[1],
                         src[2], (int)d[0], (int)d[1], (int)d[2], (int)d[3], (long)d[4], dst);
      break;
    case WP_DOT64:
      hipLaunchKernelGGL(wp_dot64_kernel<T>, dim3((unsigned)((d[0] + 255) / 256)), dim3(256), 0, s, src[0], src[1], src[2], (int)d[0], (int)d[1], dst);
      break;
    default:
      set_last_error("weight_pack: unknown kind");
      return T2P_ERR_INVALID;
  }
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

}  // namespace

// Fills in the defaulted pitches and checks the dimensions of one packing; the block it writes is [rows][width] at pitch ld
int weight_pack_shape(WeightPack& p, int64_t* rows, int64_t* width, int64_t* ld) {
  int64_t* d = p.d;
  int64_t R = 1, W = 0, L = 0;
  int nsrc = 1;
  switch (p.kind) {
    case WP_COPY:
      T2P_REQUIRE(d[0] > 0 && d[1] >= 0 && d[2] >= 0 && (d[1] > 0 || d[2] == 0), "weight_pack copy: n0 > 0, n1, n2 >= 0");
      nsrc = 1 + (d[1] > 0) + (d[2] > 0); W = d[0] + d[1] + d[2];
      break;
    case WP_ROWS:
      T2P_REQUIRE(d[0] > 0 && d[1] > 0 && (d[2] == 0 || d[2] >= d[1]), "weight_pack rows: rows, rowlen > 0, ld >= rowlen");
      if (!d[2]) d[2] = d[1];
      R = d[0]; W = d[1]; L = d[2];
      break;
    case WP_CONV3:
      T2P_REQUIRE(d[0] > 0 && d[0] <= 65535 && d[1] > 0 && (d[2] == 0 || d[2] >= d[1]), "weight_pack conv3: N, Ci > 0, cin_pad >= Ci");
      if (!d[2]) d[2] = d[1];
      T2P_REQUIRE(d[3] == 0 || d[3] >= 9 * d[2], "weight_pack conv3: ld >= 9 * cin_pad");
      if (!d[3]) d[3] = 9 * d[2];
      R = d[0]; W = 9 * d[2]; L = d[3];
      break;
    case WP_CONV3_T:
      T2P_REQUIRE(d[0] > 0 && d[1] > 0 && d[1] <= 32, "weight_pack conv3_t: N > 0, 0 < C <= 32");
      W = 9 * d[0] * d[1];
      break;
    case WP_NIN:
      T2P_REQUIRE(d[0] > 0 && d[1] > 0 && (d[2] == 1 || d[2] == 2), "weight_pack nin: K, N > 0, one or two sources");
      nsrc = (int)d[2]; W = d[2] * d[0] * d[1];
      break;
    case WP_GEGLU:
      T2P_REQUIRE(d[0] > 0 && d[1] > 0, "weight_pack geglu: inner, rowlen > 0");
      W = 2 * d[0] * d[1];
      break;
    case WP_UP4:
      T2P_REQUIRE(d[0] > 0 && d[0] <= 65535 && d[1] > 0, "weight_pack up4: co, ci > 0");
      W = 16 * d[0] * d[1];
      break;
    case WP_ADD:
      T2P_REQUIRE(d[0] > 0, "weight_pack add: n > 0");
      nsrc = 2; W = d[0];
      break;
    case WP_PRODUCT: {
      T2P_REQUIRE(d[0] > 0 && d[1] > 0 && d[2] > 0 && (d[3] == 0 || d[3] == 1), "weight_pack product: M, K, N > 0, transposed 0 / 1");
      R = d[3] ? d[2] : d[0]; W = d[3] ? d[0] : d[2];
      T2P_REQUIRE(d[4] == 0 || d[4] >= W, "weight_pack product: ld >= row width");
      if (!d[4]) d[4] = W;
      L = d[4]; nsrc = 2;
      break;
    }
    case WP_DOT64:
      T2P_REQUIRE(d[0] > 0 && d[1] > 0, "weight_pack dot64: N, K > 0");
      nsrc = 3; W = d[0];
      break;
    default:
      T2P_REQUIRE(false, "weight_pack: unknown kind");
  }
  for (int i = 0; i < nsrc; ++i) T2P_REQUIRE(p.src[i], "weight_pack: null source");
  T2P_REQUIRE(p.dst, "weight_pack: null destination");
  T2P_REQUIRE(p.dtype == DT_F32 || p.dtype == DT_F16 || p.dtype == DT_BF16, "weight_pack: bad dtype");
  *rows = R; *width = W; *ld = L ? L : W;
  return T2P_OK;
}

// bytes one packing reads (every source once) and writes, for the traffic count of a load
void weight_pack_bytes(const WeightPack& p, int64_t rows, int64_t width, int64_t* rd, int64_t* wr) {
  const int64_t* d = p.d;
  int64_t n = 0;
  switch (p.kind) {
    case WP_COPY: n = d[0] + d[1] + d[2]; break;
    case WP_ROWS: n = d[0] * d[1]; break;
    case WP_CONV3: case WP_CONV3_T: case WP_UP4: n = d[0] * d[1] * 9; break;
    case WP_NIN: n = d[0] * d[1] * d[2]; break;
    case WP_GEGLU: n = 2 * d[0] * d[1]; break;
    case WP_ADD: n = 2 * d[0]; break;
    case WP_PRODUCT: n = d[0] * d[1] + d[1] * d[2] + (p.src[2] ? d[2] : 0); break;
    case WP_DOT64: n = d[0] * d[1] + d[1] + d[0]; break;
  }
  *rd = 4 * n;
  *wr = rows * width * (int64_t)dtype_size(p.dtype);
}

int launch_weight_pack(const WeightPack& pack, hipStream_t s) {
  WeightPack p = pack;
  int64_t rows, width, ld;
  T2P_TRY(weight_pack_shape(p, &rows, &width, &ld));
  switch (p.dtype) {
    case DT_F32: return launch_typed<float>(p, s);
    case DT_BF16: return launch_typed<bf16_t>(p, s);
    default: return launch_typed<f16_t>(p, s);
  }
}

// ---- the row-resident GEMM's weights (rowgemm.hip) --------------------------------------------------------------------------------
// A packed 16-bit matrix [N][ldb] with K = 512 re-ordered (values moved, not converted) so that what a wavefront feeds one
// v_mfma_f32_16x16x32 -- 16 permuted channels x 32 k, 16 bytes per lane -- is 1 KiB contiguous, and the four column tiles of a
// 32-deep step follow one another: 16-byte piece ((slice 16 + step) 4 + j) 64 + lane.  Made once per load of the weights.
__global__ __launch_bounds__(256) void rowres_pack_kernel(const uint4* __restrict__ W, long ldb8, uint4* __restrict__ out, long npieces) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npieces) return;
  const int lane = (int)(i & 63), j = (int)((i >> 6) & 3), step = (int)((i >> 8) & 15);
  const long slice = i >> 12;
  // MFMA row 16 j + (lane & 15) of the slice is channel hperm(.) (gemm_mfma.h), written out here: r = lane & 15 -> g = r / 4, v = r % 4
  const int r = lane & 15, ch = 32 * (j >> 1) + 8 * (r >> 2) + 4 * (j & 1) + (r & 3);
  out[i] = W[(slice * 64 + ch) * ldb8 + 4 * step + (lane >> 4)];
}
int launch_rowres_pack(int dtype, const void* W, long ldb, void* out, int N, hipStream_t s) {
  T2P_REQUIRE(W && out && N > 0 && N % 64 == 0 && ldb >= 512 && ldb % 8 == 0 && (dtype == DT_F16 || dtype == DT_BF16), "rowres_pack arguments");
  T2P_REQUIRE(((uintptr_t)W % 16) == 0 && ((uintptr_t)out % 16) == 0, "rowres_pack: 16-byte aligned matrices");
  const long n = (long)N * 64;                           // 16-byte pieces of N x 512 16-bit values
  hipLaunchKernelGGL(rowres_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint4*)W, ldb / 8, (uint4*)out, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

}  // namespace t2p
