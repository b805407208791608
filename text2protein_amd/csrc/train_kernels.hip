// Kernels of the training step: fp32 storage, gfx950 only.
//
//   * tgemm16_kernel     the same strided GEMM with 16-bit products (v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulation) for the
//                        mixed-precision step: operands rounded as they are staged, split-K reduced in a fixed order
//
//   * tgemm_kernel       strided batched GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products): every product of the backward pass that
//                        is not a 3x3 convolution over pixels -- dY W, dY^T X, q k^T, P v, P^T dO, dS^T q ... -- reads its operands
//                        through (row stride, column stride) views, so nothing is transposed in memory; the weight gradient of a 3x3
//                        convolution gathers its B operand from the NHWC map (nine shifted views); split-K with hardware fp32 atomics
//                        where K is "every pixel of the batch"
//   * the backward halves of GroupNorm(+SiLU), LayerNorm, softmax, GEGLU, up / down-sampling, dropout
//   * the denoising score-matching loss of the VE SDE and its gradient (reference score_sde_pytorch/losses.py:105-131)
//   * Adam with warm-up and gradient clipping, EMA (losses.py:26-51, models/ema.py:32-49) over flat parameter buffers
//
// Layouts: activations NHWC [B][H W][C] fp32 (the inference engine's layout), the state / noise / masks NCHW as in the reference.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "philox.h"
#include "train_kernels.h"
#include "wave_reduce.h"

namespace t2p {

typedef float tg_f32x16 __attribute__((ext_vector_type(16)));

static inline int cdiv_l(long a, long b) { return (int)((a + b - 1) / b); }
static inline int grid_for(long n, int block, int cap = 65535 * 4) { return (int)std::min<long>((n + block - 1) / block, cap); }

// =====================================================================================================================================
// strided GEMM
// =====================================================================================================================================
template <int BM, int BN, bool AMC, bool BNC, bool CONVB>
__global__ __launch_bounds__(256) void tgemm_kernel(const TGemmArgs p, const int kper) {
  constexpr int BK = 16;
  constexpr int SA = BM + 32, SB = BN + 32;   // row strides = 32 mod 64 banks: the two k rows a fragment read touches never collide
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int EA = BM * BK / 256, EB = BN * BK / 256;
  __shared__ float As[BK * SA];
  __shared__ float Bs[BK * SB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
  int zz = blockIdx.z;
  const int ks = zz % p.ksplit; zz /= p.ksplit;
  const int z1 = zz % p.nz1, z0 = zz / p.nz1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kb = ks * kper, ke = min(p.K, kb + kper);

  const float* A = p.A + (long)z0 * p.sAz0 + (long)z1 * p.sAz1;
  const float* B = p.B + (long)z0 * p.sBz0 + (long)z1 * p.sBz1;

  // staging assignment
  int am, ak, akstep, amstep;
  if (AMC) { am = tid % BM; ak = tid / BM; akstep = 256 / BM; amstep = 0; }
  else     { ak = tid % BK; am = tid / BK; akstep = 0; amstep = 256 / BK; }
  int bn, bk, bkstep, bnstep;
  if (BNC) { bn = tid % BN; bk = tid / BN; bkstep = 256 / BN; bnstep = 0; }
  else     { bk = tid % BK; bn = tid / BK; bkstep = 0; bnstep = 256 / BK; }

  // convolution gather: this thread's column = (tap, channel) is fixed (BNC staging); the pixel coordinates of its EB rows are carried
  // from K-tile to K-tile (no divisions in the loop)
  int cv_c = 0, cv_dy = 0, cv_dx = 0;
  bool cv_ok = false;
  int cv_b[CONVB ? EB : 1], cv_y[CONVB ? EB : 1], cv_x[CONVB ? EB : 1];
  if (CONVB) {
    const int HW = p.H * p.W;
    const int gn = n0 + bn;
    cv_ok = gn < p.N;
    const int tap = cv_ok ? gn / p.conv_C : 0;
    cv_c = gn - tap * p.conv_C;
    cv_dy = tap / 3 - 1;
    cv_dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
    for (int i = 0; i < EB; ++i) {
      const int gk = kb + bk + i * bkstep;
      cv_b[i] = gk / HW;
      const int rem = gk - cv_b[i] * HW;
      cv_y[i] = rem / p.W;
      cv_x[i] = rem - cv_y[i] * p.W;
    }
  }

  tg_f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  for (int k0 = kb; k0 < ke; k0 += BK) {
    float ra[EA], rb[EB];
#pragma unroll
    for (int i = 0; i < EA; ++i) {
      const int m = am + i * amstep, k = ak + i * akstep;
      const int gm = m0 + m, gk = k0 + k;
      ra[i] = (gm < p.M && gk < ke) ? A[(long)gm * p.sAm + (long)gk * p.sAk] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < EB; ++i) {
      const int n = bn + i * bnstep, k = bk + i * bkstep;
      const int gn = n0 + n, gk = k0 + k;
      float v = 0.f;
      if (CONVB) {
        if (cv_ok && gk < ke) {
          const int sy = cv_y[i] + cv_dy, sx = cv_x[i] + cv_dx;
          if (sy >= 0 && sy < p.H && sx >= 0 && sx < p.W) v = B[((long)(cv_b[i] * p.H + sy) * p.W + sx) * p.ldx + cv_c];
        }
        cv_x[i] += BK;                      // the row this slot stages in the next K-tile
        while (cv_x[i] >= p.W) { cv_x[i] -= p.W; ++cv_y[i]; }
        while (cv_y[i] >= p.H) { cv_y[i] -= p.H; ++cv_b[i]; }
      } else if (gn < p.N && gk < ke) {
        v = B[(long)gk * p.sBk + (long)gn * p.sBn];
      }
      rb[i] = v;
    }
    __syncthreads();     // the previous K-tile has been consumed
#pragma unroll
    for (int i = 0; i < EA; ++i) As[(ak + i * akstep) * SA + am + i * amstep] = ra[i];
#pragma unroll
    for (int i = 0; i < EB; ++i) Bs[(bk + i * bkstep) * SB + bn + i * bnstep] = rb[i];
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = As[(kk + lh) * SA + wm * (BM / 2) + i * 32 + lr];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = Bs[(kk + lh) * SB + wn * (BN / 2) + j * 32 + lr];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }

  float* C = p.C + (long)z0 * p.sCz0 + (long)z1 * p.sCz1;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = m0 + wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
      if (row >= p.M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * (BN / 2) + j * 32 + lr;
        if (col >= p.N) continue;
        float val = p.alpha * acc[i][j][v];
        float* dst = C + (long)row * p.ldc + col;
        if (p.ksplit > 1) {
          if (ks == 0 && p.bias_n) val += p.bias_n[col];
          unsafeAtomicAdd(dst, val);
        } else {
          if (p.bias_n) val += p.bias_n[col];
          if (p.beta != 0.f) val += p.beta * *dst;
          *dst = val;
        }
      }
    }
}

template <int BT, bool AMC, bool BNC, bool CONVB>
static int tgemm_launch_t(const TGemmArgs& a, int ksplit, hipStream_t s) {
  TGemmArgs p = a;
  p.ksplit = ksplit;
  int kper = (a.K + ksplit - 1) / ksplit;
  kper = (kper + 15) / 16 * 16;
  dim3 grid(cdiv_l(a.N, BT), cdiv_l(a.M, BT), a.nz0 * a.nz1 * ksplit);
  hipLaunchKernelGGL((tgemm_kernel<BT, BT, AMC, BNC, CONVB>), grid, dim3(256), 0, s, p, kper);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

int launch_tgemm(const TGemmArgs& a, hipStream_t s) {
  T2P_REQUIRE(a.A && a.B && a.C && a.M > 0 && a.N > 0 && a.K > 0 && a.nz0 >= 1 && a.nz1 >= 1, "tgemm operands");
  T2P_REQUIRE(a.sAm == 1 || a.sAk == 1, "tgemm: A must be a row- or column-major view");
  T2P_REQUIRE(a.conv_b || a.sBn == 1 || a.sBk == 1, "tgemm: B must be a row- or column-major view");
  T2P_REQUIRE(a.ldc >= a.N, "tgemm: ldc");
  if (a.conv_b) T2P_REQUIRE(a.H > 0 && a.W > 0 && a.conv_C > 0 && a.N == 9 * a.conv_C && a.K % (a.H * a.W) == 0 && a.ldx >= a.conv_C,
                            "tgemm: convolution gather shapes");
  const long nz = (long)a.nz0 * a.nz1;
  T2P_REQUIRE(nz <= 65535, "tgemm: batch count");
  // 128 x 128 tiles when they fill the chip by themselves -- or together with the K splits this call may choose (weight gradients)
  const long tiles128 = (long)cdiv_l(a.M, 128) * cdiv_l(a.N, 128) * nz;
  const bool big = a.M >= 128 && a.N >= 128 && (tiles128 >= 128 || (a.ksplit == 0 && tiles128 * (a.K / 256) >= 128));
  const int bt = big ? 128 : 64;
  int ksplit = a.ksplit;
  if (ksplit == 0) {
    const long tiles = (long)cdiv_l(a.M, bt) * cdiv_l(a.N, bt) * nz;
    ksplit = (int)std::max<long>(1, std::min<long>(512 / std::max<long>(tiles, 1), a.K / 256));
  }
  T2P_REQUIRE(ksplit >= 1 && nz * ksplit <= 65535, "tgemm: ksplit");
  T2P_REQUIRE(ksplit == 1 || a.beta == 1.f, "tgemm: split-K accumulates with atomics and needs beta == 1");
  const bool amc = a.sAm == 1, bnc = a.conv_b || a.sBn == 1;
  if (a.conv_b) {
    T2P_REQUIRE(amc, "tgemm: the convolution weight gradient takes dY^T (column-major view) as A");
    return big ? tgemm_launch_t<128, true, true, true>(a, ksplit, s) : tgemm_launch_t<64, true, true, true>(a, ksplit, s);
  }
#define T2P_TG(AM, BN_)                                                                                     \
  if (amc == AM && bnc == BN_)                                                                              \
    return big ? tgemm_launch_t<128, AM, BN_, false>(a, ksplit, s) : tgemm_launch_t<64, AM, BN_, false>(a, ksplit, s);
  T2P_TG(true, true) T2P_TG(true, false) T2P_TG(false, true) T2P_TG(false, false)
#undef T2P_TG
  return T2P_ERR_INVALID;
}

// =====================================================================================================================================
// strided GEMM, 16-bit products (mixed-precision training step): the same TGemmArgs views, batches, epilogue and convolution gather
// as tgemm_kernel; the fp32 operands are rounded to f16 / bf16 (round to nearest even, no saturation: an overflow becomes +-inf) while
// they are staged into LDS and multiplied on v_mfma_f32_32x32x16_{f16,bf16} with fp32 accumulation.
//   * LDS holds both tiles K-contiguous, [row][BK + 8] 16-bit elements: one ds_read_b128 per 32 x 16 fragment, an 80-byte row pitch
//     (20 banks) keeps the eight rows a 16-byte read phase touches on disjoint banks
//   * a thread stages 8 consecutive k of one row (one 16-byte LDS store); along the contiguous global dimension the lanes of a wave
//     read neighbouring addresses (m- / n-contiguous views), or each lane reads two float4 (k-contiguous views that are 16-byte aligned)
//   * split-K writes raw partial tiles to a workspace [ks][z][M][N]; tgemm16_reduce_kernel sums them in ks order and applies the
//     epilogue, so the result does not depend on the order in which workgroups finish (no atomics: bitwise reproducible)
// =====================================================================================================================================
template <typename TC> __device__ inline uint4 tg_pack8(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t lo, hi;
    if constexpr (sizeof(TC) == 2 && dtype_of<TC>::value == DT_F16) {
      lo = __builtin_bit_cast(uint16_t, (_Float16)f[2 * i]);
      hi = __builtin_bit_cast(uint16_t, (_Float16)f[2 * i + 1]);
    } else {
      lo = f32_to_bf16_bits(f[2 * i]);
      hi = f32_to_bf16_bits(f[2 * i + 1]);
    }
    w[i] = (uint32_t)lo | ((uint32_t)hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

typedef _Float16 tg_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 tg_bf16x8 __attribute__((ext_vector_type(8)));
template <typename TC> __device__ inline void tg_mma16(const uint4& a, const uint4& b, tg_f32x16& c) {
  if constexpr (dtype_of<TC>::value == DT_F16)
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tg_f16x8, a), __builtin_bit_cast(tg_f16x8, b), c, 0, 0, 0);
  else
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(tg_bf16x8, a), __builtin_bit_cast(tg_bf16x8, b), c, 0, 0, 0);
}

template <typename TC, int BM, int BN, bool AMC, bool BNC, bool CONVB>
__global__ __launch_bounds__(256) void tgemm16_kernel(const TGemmArgs p, const int kper, float* __restrict__ ws, const int vec_a,
                                                      const int vec_b) {
  constexpr int BK = 32, LDK = BK + 8;
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int EA = BM * BK / (256 * 8), EB = BN * BK / (256 * 8);   // 8-element k-groups staged per thread
  __shared__ __attribute__((aligned(16))) uint16_t As[BM * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[BN * LDK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
  int zz = blockIdx.z;
  const int ks = zz % p.ksplit; zz /= p.ksplit;
  const int z1 = zz % p.nz1, z0 = zz / p.nz1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kb = ks * kper, ke = min(p.K, kb + kper);

  const float* A = p.A + (long)z0 * p.sAz0 + (long)z1 * p.sAz1;
  const float* B = p.B + (long)z0 * p.sBz0 + (long)z1 * p.sBz1;
  const int HW = p.H * p.W;

  tg_f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  // staging slots of this thread: item e = (row r / column n, k-group q); fixed for the whole K loop
  int ar[EA], aq[EA], bnl[EB], bq[EB];
#pragma unroll
  for (int e = 0; e < EA; ++e) {
    const int idx = tid + 256 * e;
    ar[e] = AMC ? idx % BM : idx / 4; aq[e] = AMC ? idx / BM : idx % 4;
  }
  constexpr bool NCONT = BNC || CONVB;
#pragma unroll
  for (int e = 0; e < EB; ++e) {
    const int idx = tid + 256 * e;
    bnl[e] = NCONT ? idx % BN : idx / 4; bq[e] = NCONT ? idx / BN : idx % 4;
  }
  // convolution gather: the column (tap, channel) of a slot is fixed; the pixel (b, y, x) of its first k is carried from K-tile to K-tile
  // (divisions only here)
  int cv_c[CONVB ? EB : 1], cv_dy[CONVB ? EB : 1], cv_dx[CONVB ? EB : 1], cv_b[CONVB ? EB : 1], cv_y[CONVB ? EB : 1], cv_x[CONVB ? EB : 1];
  if (CONVB) {
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int gn = n0 + bnl[e];
      const int tap = gn < p.N ? gn / p.conv_C : 0;
      cv_c[e] = gn - tap * p.conv_C;
      cv_dy[e] = tap / 3 - 1;
      cv_dx[e] = tap - (tap / 3) * 3 - 1;
      const int gk = kb + 8 * bq[e];
      cv_b[e] = gk / HW;
      const int rem = gk - cv_b[e] * HW;
      cv_y[e] = rem / p.W;
      cv_x[e] = rem - cv_y[e] * p.W;
    }
  }

  // global -> registers (fp32, not yet rounded: the loads of K-tile t + 1 stay in flight while tile t is multiplied)
  float fa[EA][8], fb[EB][8];
  auto gload = [&](const int k0) {
#pragma unroll
    for (int e = 0; e < EA; ++e) {
      const int gm = m0 + ar[e], gk = k0 + 8 * aq[e];
      if (!AMC && vec_a && gm < p.M && gk + 8 <= ke) {
        const float4* src = (const float4*)(A + (long)gm * p.sAm + gk);
        const float4 x = src[0], y = src[1];
        fa[e][0] = x.x; fa[e][1] = x.y; fa[e][2] = x.z; fa[e][3] = x.w; fa[e][4] = y.x; fa[e][5] = y.y; fa[e][6] = y.z; fa[e][7] = y.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) fa[e][j] = (gm < p.M && gk + j < ke) ? A[(long)gm * p.sAm + (long)(gk + j) * p.sAk] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int gn = n0 + bnl[e], gk = k0 + 8 * bq[e];
      if (CONVB) {
        // B(k = output pixel, n = tap conv_C + c) = X[pixel + offset(tap)][c], zero outside the map
        const int sy = cv_y[e] + cv_dy[e], sx = cv_x[e] + cv_dx[e];
        const bool ok = gn < p.N && gk + 8 <= ke;
        if (ok && cv_x[e] + 8 <= p.W && sy >= 0 && sy < p.H && sx >= 0 && sx + 8 <= p.W) {
          // the 8 pixels lie in one row, inside the map: plain strided loads
          const float* src = B + ((long)(cv_b[e] * p.H + sy) * p.W + sx) * p.ldx + cv_c[e];
#pragma unroll
          for (int j = 0; j < 8; ++j) fb[e][j] = src[(long)j * p.ldx];
        } else {
          int b = cv_b[e], y = cv_y[e], x = cv_x[e];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int yy = y + cv_dy[e], xx = x + cv_dx[e];
            fb[e][j] = (gn < p.N && gk + j < ke && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W)
                           ? B[((long)(b * p.H + yy) * p.W + xx) * p.ldx + cv_c[e]] : 0.f;
            if (++x == p.W) { x = 0; if (++y == p.H) { y = 0; ++b; } }
          }
        }
        cv_x[e] += BK;                      // the first pixel this slot stages in the next K-tile
        while (cv_x[e] >= p.W) { cv_x[e] -= p.W; if (++cv_y[e] == p.H) { cv_y[e] = 0; ++cv_b[e]; } }
      } else if (!BNC && vec_b && gn < p.N && gk + 8 <= ke) {
        const float4* src = (const float4*)(B + gk + (long)gn * p.sBn);
        const float4 x = src[0], y = src[1];
        fb[e][0] = x.x; fb[e][1] = x.y; fb[e][2] = x.z; fb[e][3] = x.w; fb[e][4] = y.x; fb[e][5] = y.y; fb[e][6] = y.z; fb[e][7] = y.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) fb[e][j] = (gn < p.N && gk + j < ke) ? B[(long)(gk + j) * p.sBk + (long)gn * p.sBn] : 0.f;
      }
    }
  };

  if (kb < ke) gload(kb);
  for (int k0 = kb; k0 < ke; k0 += BK) {
    uint4 ra[EA], rb[EB];
#pragma unroll
    for (int e = 0; e < EA; ++e) ra[e] = tg_pack8<TC>(fa[e]);
#pragma unroll
    for (int e = 0; e < EB; ++e) rb[e] = tg_pack8<TC>(fb[e]);
    __syncthreads();     // the previous K-tile has been consumed
#pragma unroll
    for (int e = 0; e < EA; ++e) *(uint4*)&As[ar[e] * LDK + 8 * aq[e]] = ra[e];
#pragma unroll
    for (int e = 0; e < EB; ++e) *(uint4*)&Bs[bnl[e] * LDK + 8 * bq[e]] = rb[e];
    __syncthreads();
    if (k0 + BK < ke) gload(k0 + BK);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      uint4 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *(const uint4*)&As[(wm * (BM / 2) + i * 32 + lr) * LDK + 16 * s + 8 * lh];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = *(const uint4*)&Bs[(wn * (BN / 2) + j * 32 + lr) * LDK + 16 * s + 8 * lh];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) tg_mma16<TC>(af[i], bf[j], acc[i][j]);
    }
  }

  float* C = p.C + (long)z0 * p.sCz0 + (long)z1 * p.sCz1;
  float* part = p.ksplit > 1 ? ws + ((long)ks * p.nz0 * p.nz1 + (long)z0 * p.nz1 + z1) * p.M * p.N : nullptr;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = m0 + wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
      if (row >= p.M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * (BN / 2) + j * 32 + lr;
        if (col >= p.N) continue;
        if (part) {
          part[(long)row * p.N + col] = acc[i][j][v];
        } else {
          float val = p.alpha * acc[i][j][v];
          float* dst = C + (long)row * p.ldc + col;
          if (p.bias_n) val += p.bias_n[col];
          if (p.beta != 0.f) val += p.beta * *dst;
          *dst = val;
        }
      }
    }
}

// C = alpha (sum over ks of the partial tiles, in ks order) + bias_n + beta C
__global__ __launch_bounds__(256) void tgemm16_reduce_kernel(const TGemmArgs p, const float* __restrict__ ws, const int ksplit) {
  const long MN = (long)p.M * p.N, total = MN * p.nz0 * p.nz1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    float s = 0.f;
    for (int k = 0; k < ksplit; ++k) s += ws[k * total + i];
    const long z = i / MN, e = i - z * MN;
    const int row = (int)(e / p.N), col = (int)(e - (long)row * p.N);
    const int z0 = (int)(z / p.nz1), z1 = (int)(z - (long)z0 * p.nz1);
    float* dst = p.C + (long)z0 * p.sCz0 + (long)z1 * p.sCz1 + (long)row * p.ldc + col;
    float val = p.alpha * s;
    if (p.bias_n) val += p.bias_n[col];
    if (p.beta != 0.f) val += p.beta * *dst;
    *dst = val;
  }
}

// tile edge and K split of a 16-bit launch: the f32 rule with the 32-deep K-tile
static void tgemm16_plan(const TGemmArgs& a, int* bt, int* ksplit) {
  const long nz = (long)a.nz0 * a.nz1;
  const long tiles128 = (long)cdiv_l(a.M, 128) * cdiv_l(a.N, 128) * nz;
  const bool big = a.M >= 128 && a.N >= 128 && (tiles128 >= 128 || (a.ksplit == 0 && tiles128 * (a.K / 256) >= 128));
  *bt = big ? 128 : 64;
  int ks = a.ksplit;
  if (ks == 0) {
    const long tiles = (long)cdiv_l(a.M, *bt) * cdiv_l(a.N, *bt) * nz;
    ks = (int)std::max<long>(1, std::min<long>(512 / std::max<long>(tiles, 1), a.K / 256));
  }
  *ksplit = ks;
}

long tgemm16_ws_floats(const TGemmArgs& a) {
  int bt = 0, ks = 1;
  tgemm16_plan(a, &bt, &ks);
  return ks > 1 ? (long)ks * a.nz0 * a.nz1 * a.M * a.N : 0;
}

template <typename TC, int BT, bool AMC, bool BNC, bool CONVB>
static int tgemm16_launch_t(const TGemmArgs& a, int ksplit, float* ws, int vec_a, int vec_b, hipStream_t s) {
  TGemmArgs p = a;
  p.ksplit = ksplit;
  int kper = (a.K + ksplit - 1) / ksplit;
  kper = (kper + 31) / 32 * 32;
  dim3 grid(cdiv_l(a.N, BT), cdiv_l(a.M, BT), a.nz0 * a.nz1 * ksplit);
  hipLaunchKernelGGL((tgemm16_kernel<TC, BT, BT, AMC, BNC, CONVB>), grid, dim3(256), 0, s, p, kper, ws, vec_a, vec_b);
  T2P_HIP_CHECK(hipGetLastError());
  if (ksplit > 1) {
    const long total = (long)a.M * a.N * a.nz0 * a.nz1;
    hipLaunchKernelGGL(tgemm16_reduce_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, p, (const float*)ws, ksplit);
    T2P_HIP_CHECK(hipGetLastError());
  }
  return T2P_OK;
}

template <typename TC>
static int tgemm16_dispatch(const TGemmArgs& a, int bt, int ksplit, float* ws, int vec_a, int vec_b, hipStream_t s) {
  const bool amc = a.sAm == 1, bnc = a.sBn == 1;
  if (a.conv_b)
    return bt == 128 ? tgemm16_launch_t<TC, 128, true, true, true>(a, ksplit, ws, 0, 0, s)
                     : tgemm16_launch_t<TC, 64, true, true, true>(a, ksplit, ws, 0, 0, s);
#define T2P_TG16(AM, BN_)                                                                                   \
  if (amc == AM && bnc == BN_)                                                                              \
    return bt == 128 ? tgemm16_launch_t<TC, 128, AM, BN_, false>(a, ksplit, ws, vec_a, vec_b, s)            \
                     : tgemm16_launch_t<TC, 64, AM, BN_, false>(a, ksplit, ws, vec_a, vec_b, s);
  T2P_TG16(true, true) T2P_TG16(true, false) T2P_TG16(false, true) T2P_TG16(false, false)
#undef T2P_TG16
  return T2P_ERR_INVALID;
}

int launch_tgemm16(const TGemmArgs& a, int dtype, float* ws, hipStream_t s) {
  T2P_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "tgemm16: dtype must be f16 or bf16");
  T2P_REQUIRE(a.A && a.B && a.C && a.M > 0 && a.N > 0 && a.K > 0 && a.nz0 >= 1 && a.nz1 >= 1, "tgemm operands");
  T2P_REQUIRE(a.sAm == 1 || a.sAk == 1, "tgemm: A must be a row- or column-major view");
  T2P_REQUIRE(a.conv_b || a.sBn == 1 || a.sBk == 1, "tgemm: B must be a row- or column-major view");
  T2P_REQUIRE(a.ldc >= a.N, "tgemm: ldc");
  if (a.conv_b) T2P_REQUIRE(a.H > 0 && a.W > 0 && a.conv_C > 0 && a.N == 9 * a.conv_C && a.K % (a.H * a.W) == 0 && a.ldx >= a.conv_C,
                            "tgemm: convolution gather shapes");
  if (a.conv_b) T2P_REQUIRE(a.sAm == 1, "tgemm: the convolution weight gradient takes dY^T (column-major view) as A");
  const long nz = (long)a.nz0 * a.nz1;
  T2P_REQUIRE(nz <= 65535, "tgemm: batch count");
  int bt = 64, ksplit = 1;
  tgemm16_plan(a, &bt, &ksplit);
  T2P_REQUIRE(ksplit >= 1 && nz * ksplit <= 65535, "tgemm: ksplit");
  T2P_REQUIRE(ksplit == 1 || ws, "tgemm16: a split-K launch needs its workspace (tgemm16_ws_floats)");
  T2P_REQUIRE((long)ksplit * nz * a.M * a.N < (1L << 40), "tgemm16: workspace size");
  // two float4 per staged k-group: the k-contiguous operand rows must start on 16 bytes
  auto aligned = [](const float* p, long s1, long s2, long s3) {
    return ((uintptr_t)p % 16) == 0 && s1 % 4 == 0 && s2 % 4 == 0 && s3 % 4 == 0;
  };
  const int vec_a = a.sAk == 1 && aligned(a.A, a.sAm, a.sAz0, a.sAz1);
  const int vec_b = !a.conv_b && a.sBk == 1 && aligned(a.B, a.sBn, a.sBz0, a.sBz1);
  return dtype == DT_F16 ? tgemm16_dispatch<f16_t>(a, bt, ksplit, ws, vec_a, vec_b, s)
                         : tgemm16_dispatch<bf16_t>(a, bt, ksplit, ws, vec_a, vec_b, s);
}

// =====================================================================================================================================
// reductions shared below: wave_sum comes from wave_reduce.h
// =====================================================================================================================================
__device__ inline float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }

// =====================================================================================================================================
// GroupNorm backward
// =====================================================================================================================================
constexpr int GN_CHUNK = 64;   // pixels per partial-sum block

// ws_partial [B][nchunk][C][2] = per-chunk (sum dv, sum dv n)
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const int silu, const int HW, const int C,
                                                             const int G, float* __restrict__ ws) {
  __shared__ float red[2][256];
  const int b = blockIdx.y, ch = blockIdx.x, nchunk = gridDim.x, tid = threadIdx.x;
  const int p0 = ch * GN_CHUNK, p1 = min(HW, p0 + GN_CHUNK);
  const int cg = C / G;
  const int PL = (C < 256 && 256 % C == 0) ? 256 / C : 1;   // pixel lanes when the channels do not fill the block
  const int cl = PL > 1 ? tid % C : tid, pl = PL > 1 ? tid / C : 0;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int c = c0 + cl;
    float a = 0.f, bq = 0.f;
    if (c < C) {
      const int g = c / cg;
      const float mean = stats[((long)b * G + g) * 2], rstd = stats[((long)b * G + g) * 2 + 1];
      const float ga = gamma[c], be = beta[c];
      for (int p = p0 + pl; p < p1; p += PL) {
        const long i = ((long)b * HW + p) * C + c;
        const float n = (x[i] - mean) * rstd;
        float dv = dy[i];
        if (silu) {
          const float v = n * ga + be, sg = sigmoidf_(v);
          dv *= sg * (1.f + v * (1.f - sg));
        }
        a += dv;
        bq += dv * n;
      }
    }
    if (PL > 1) {
      red[0][tid] = a; red[1][tid] = bq;
      __syncthreads();
      if (pl == 0) {
        for (int q = 1; q < PL; ++q) { a += red[0][q * C + cl]; bq += red[1][q * C + cl]; }
      }
      __syncthreads();
    }
    if (c < C && pl == 0) {
      float* o = ws + (((long)b * nchunk + ch) * C + c) * 2;
      o[0] = a; o[1] = bq;
    }
  }
}

// per sample: fold the chunks -> sums [B][C][2], group sums gs [B][G][2] = (sum gamma dv, sum gamma dv n); dgamma / dbeta += over the batch
template <bool ATOMIC>   // false: dgamma / dbeta are left to gn_bwd_param_sum_kernel (fixed order over the batch)
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ gamma,
                                                              const int nchunk, const int C, const int G, float* __restrict__ sums,
                                                              float* __restrict__ gs, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int b = blockIdx.x, tid = threadIdx.x, cg = C / G;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f, bq = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) {
      const float* o = partial + (((long)b * nchunk + ch) * C + c) * 2;
      a += o[0]; bq += o[1];
    }
    sums[((long)b * C + c) * 2] = a;
    sums[((long)b * C + c) * 2 + 1] = bq;
    if (ATOMIC) {
      unsafeAtomicAdd(dbeta + c, a);
      unsafeAtomicAdd(dgamma + c, bq);
    }
  }
  __syncthreads();
  for (int g = tid; g < G; g += 256) {
    float s1 = 0.f, s2 = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
      s1 += gamma[c] * sums[((long)b * C + c) * 2];
      s2 += gamma[c] * sums[((long)b * C + c) * 2 + 1];
    }
    gs[((long)b * G + g) * 2] = s1;
    gs[((long)b * G + g) * 2 + 1] = s2;
  }
}

__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const int silu, const int HW, const int C, const int G,
                                                           const float* __restrict__ gs, float* __restrict__ dx, const long total) {
  const int cg = C / G;
  const float inv_m = 1.f / ((float)HW * cg);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long bp = i / C;
    const int b = (int)(bp / HW), g = c / cg;
    const float mean = stats[((long)b * G + g) * 2], rstd = stats[((long)b * G + g) * 2 + 1];
    const float ga = gamma[c];
    const float n = (x[i] - mean) * rstd;
    float dv = dy[i];
    if (silu) {
      const float v = n * ga + beta[c], sg = sigmoidf_(v);
      dv *= sg * (1.f + v * (1.f - sg));
    }
    const float s1 = gs[((long)b * G + g) * 2], s2 = gs[((long)b * G + g) * 2 + 1];
    dx[i] += rstd * (dv * ga - (s1 + n * s2) * inv_m);
  }
}

long gn_bwd_ws_floats(int B, int HW, int C, int G) {
  const long nchunk = (HW + GN_CHUNK - 1) / GN_CHUNK;
  return (long)B * nchunk * C * 2 + (long)B * C * 2 + (long)B * G * 2;
}

// fixed order: d gamma / d beta = the per-sample sums added over the batch in sample order
__global__ __launch_bounds__(256) void gn_bwd_param_sum_kernel(const float* __restrict__ sums, const int B, const int C, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, bq = 0.f;
  for (int b = 0; b < B; ++b) { a += sums[((long)b * C + c) * 2]; bq += sums[((long)b * C + c) * 2 + 1]; }
  dbeta[c] += a;
  dgamma[c] += bq;
}

int launch_gn_backward(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta, int silu,
                       int B, int HW, int C, int G, float* dx, float* dgamma, float* dbeta, float* ws, bool fixed_order, hipStream_t s) {
  T2P_REQUIRE(x && dy && stats && gamma && beta && dx && dgamma && dbeta && ws, "gn_backward pointers");
  T2P_REQUIRE(B > 0 && HW > 0 && C > 0 && G > 0 && C % G == 0 && B <= 65535, "gn_backward shapes");
  const int nchunk = (HW + GN_CHUNK - 1) / GN_CHUNK;
  float* partial = ws;
  float* sums = partial + (long)B * nchunk * C * 2;
  float* gs = sums + (long)B * C * 2;
  hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3(nchunk, B), dim3(256), 0, s, x, dy, stats, gamma, beta, silu, HW, C, G, partial);
  if (fixed_order) {
    hipLaunchKernelGGL(gn_bwd_finalize_kernel<false>, dim3(B), dim3(256), 0, s, partial, gamma, nchunk, C, G, sums, gs, dgamma, dbeta);
    hipLaunchKernelGGL(gn_bwd_param_sum_kernel, dim3(cdiv_l(C, 256)), dim3(256), 0, s, (const float*)sums, B, C, dgamma, dbeta);
  } else {
    hipLaunchKernelGGL(gn_bwd_finalize_kernel<true>, dim3(B), dim3(256), 0, s, partial, gamma, nchunk, C, G, sums, gs, dgamma, dbeta);
  }
  const long total = (long)B * HW * C;
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, x, dy, stats, gamma, beta, silu, HW, C, G, gs, dx, total);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// =====================================================================================================================================
// LayerNorm backward: one wavefront per row, per-block channel sums in LDS
// =====================================================================================================================================
constexpr int LN_ROWS = 64;   // rows per block

__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gamma,
                                                     const long rows, const int C, const float eps, float* __restrict__ dx,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  extern __shared__ float ln_sh[];     // [2][C]
  float* sg = ln_sh;
  float* sb = ln_sh + C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < C; c += 256) { sg[c] = 0.f; sb[c] = 0.f; }
  __syncthreads();
  const long r0 = (long)blockIdx.x * LN_ROWS, r1 = min(rows, r0 + LN_ROWS);
  const float inv_c = 1.f / C;
  for (long r = r0 + wave; r < r1; r += 4) {
    const float* xr = x + r * C;
    const float* dr = dy + r * C;
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += xr[c];
    const float mean = wave_sum(sum) * inv_c;
    float var = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; var += d * d; }
    const float rstd = rsqrtf(wave_sum(var) * inv_c + eps);
    float c1 = 0.f, c2 = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float n = (xr[c] - mean) * rstd, dg = dr[c] * gamma[c];
      c1 += dg; c2 += dg * n;
    }
    c1 = wave_sum(c1) * inv_c; c2 = wave_sum(c2) * inv_c;
    for (int c = lane; c < C; c += 64) {
      const float n = (xr[c] - mean) * rstd, d = dr[c];
      dx[r * C + c] += rstd * (d * gamma[c] - c1 - n * c2);
      atomicAdd(sg + c, d * n);      // LDS atomics (ds_add_f32)
      atomicAdd(sb + c, d);
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    unsafeAtomicAdd(dgamma + c, sg[c]);
    unsafeAtomicAdd(dbeta + c, sb[c]);
  }
}

// the same in a fixed summation order (mixed-precision step, which is bitwise reproducible): pass 1 = one wavefront per row, dx and the
// row's (mean, rstd); pass 2 = per chunk of LN_COL_ROWS rows one thread per channel sums d gamma / d beta in row order; pass 3 adds the
// chunks in order
constexpr int LN_COL_ROWS = 256;
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gamma,
                                                          const long rows, const int C, const float eps, float* __restrict__ dx,
                                                          float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float inv_c = 1.f / C;
  const float* xr = x + r * C;
  const float* dr = dy + r * C;
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += xr[c];
  const float mean = wave_sum(sum) * inv_c;
  float var = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; var += d * d; }
  const float rstd = rsqrtf(wave_sum(var) * inv_c + eps);
  float c1 = 0.f, c2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float n = (xr[c] - mean) * rstd, dg = dr[c] * gamma[c];
    c1 += dg; c2 += dg * n;
  }
  c1 = wave_sum(c1) * inv_c; c2 = wave_sum(c2) * inv_c;
  for (int c = lane; c < C; c += 64) {
    const float n = (xr[c] - mean) * rstd;
    dx[r * C + c] += rstd * (dr[c] * gamma[c] - c1 - n * c2);
  }
  if (lane == 0) { stats[2 * r] = mean; stats[2 * r + 1] = rstd; }
}
__global__ __launch_bounds__(256) void ln_bwd_cols_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ stats,
                                                          const long rows, const int C, float* __restrict__ partial) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const long r0 = (long)blockIdx.y * LN_COL_ROWS, r1 = min(rows, r0 + LN_COL_ROWS);
  float g = 0.f, b = 0.f;
  for (long r = r0; r < r1; ++r) {
    const float d = dy[r * C + c];
    g += d * ((x[r * C + c] - stats[2 * r]) * stats[2 * r + 1]);
    b += d;
  }
  partial[(long)blockIdx.y * 2 * C + c] = g;
  partial[(long)blockIdx.y * 2 * C + C + c] = b;
}
__global__ __launch_bounds__(256) void ln_bwd_cols_finish_kernel(const float* __restrict__ partial, const int nchunk, const int C,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float g = 0.f, b = 0.f;
  for (int k = 0; k < nchunk; ++k) { g += partial[(long)k * 2 * C + c]; b += partial[(long)k * 2 * C + C + c]; }
  dgamma[c] += g;
  dbeta[c] += b;
}
long ln_bwd_ws_floats(long rows, int C) { return 2 * rows + 2L * C * cdiv_l(rows, LN_COL_ROWS); }
int launch_ln_backward(const float* x, const float* dy, const float* gamma, long rows, int C, float eps, float* dx, float* dgamma,
                       float* dbeta, float* ws, hipStream_t s) {
  T2P_REQUIRE(x && dy && gamma && dx && dgamma && dbeta && rows > 0 && C > 0, "ln_backward arguments");
  if (!ws) {
    T2P_REQUIRE(C <= 8192, "ln_backward arguments");
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(cdiv_l(rows, LN_ROWS)), dim3(256), 2 * C * sizeof(float), s, x, dy, gamma, rows, C, eps, dx, dgamma, dbeta);
  } else {
    const int nchunk = cdiv_l(rows, LN_COL_ROWS);
    T2P_REQUIRE(nchunk <= 65535, "ln_backward rows");
    float* stats = ws;
    float* partial = ws + 2 * rows;
    hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3(cdiv_l(rows, 4)), dim3(256), 0, s, x, dy, gamma, rows, C, eps, dx, stats);
    hipLaunchKernelGGL(ln_bwd_cols_kernel, dim3(cdiv_l(C, 256), nchunk), dim3(256), 0, s, x, dy, (const float*)stats, rows, C, partial);
    hipLaunchKernelGGL(ln_bwd_cols_finish_kernel, dim3(cdiv_l(C, 256)), dim3(256), 0, s, (const float*)partial, nchunk, C, dgamma, dbeta);
  }
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// =====================================================================================================================================
// softmax / GEGLU backward, elementwise
// =====================================================================================================================================
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, const long rows, const int n,
                                                          const float scale) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* pr = P + r * n;
  float* dr = dP + r * n;
  float dot = 0.f;
  for (int j = lane; j < n; j += 64) dot += pr[j] * dr[j];
  dot = wave_sum(dot);
  for (int j = lane; j < n; j += 64) dr[j] = scale * pr[j] * (dr[j] - dot);
}
int launch_softmax_backward(const float* P, float* dP, long rows, int n, float scale, hipStream_t s) {
  T2P_REQUIRE(P && dP && rows > 0 && n > 0, "softmax_backward arguments");
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3(cdiv_l(rows, 4)), dim3(256), 0, s, P, dP, rows, n, scale);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void geglu_bwd_kernel(const float* __restrict__ u, const float* __restrict__ dy, float* __restrict__ du,
                                                        const long rows, const int inner) {
  const long total = rows * inner;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / inner;
    const int j = (int)(i - r * inner);
    const float a = u[r * 2 * inner + j], g = u[r * 2 * inner + inner + j], d = dy[i];
    const float cdf = 0.5f * (1.f + erff(g * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * g * g);
    du[r * 2 * inner + j] += d * g * cdf;
    du[r * 2 * inner + inner + j] += d * a * (cdf + g * pdf);
  }
}
int launch_geglu_backward(const float* u, const float* dy, float* du, long rows, int inner, hipStream_t s) {
  T2P_REQUIRE(u && dy && du && rows > 0 && inner > 0, "geglu_backward arguments");
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3(grid_for(rows * inner, 256)), dim3(256), 0, s, u, dy, du, rows, inner);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

template <int OP>   // 0 silu, 1 silu backward (+=), 2 axpy, 3 add_scale
__global__ __launch_bounds__(256) void ew_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                 const float alpha, const long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    if (OP == 0) { const float v = a[i]; out[i] = v * sigmoidf_(v); }
    if (OP == 1) { const float v = a[i], sg = sigmoidf_(v); out[i] += b[i] * sg * (1.f + v * (1.f - sg)); }
    if (OP == 2) out[i] += alpha * a[i];
    if (OP == 3) out[i] = alpha * (a[i] + b[i]);
  }
}
int launch_silu(const float* x, float* y, long n, hipStream_t s) {
  T2P_REQUIRE(x && y && n > 0, "silu arguments");
  hipLaunchKernelGGL(ew_kernel<0>, dim3(grid_for(n, 256)), dim3(256), 0, s, x, nullptr, y, 0.f, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
int launch_silu_backward(const float* x, const float* dy, float* dx, long n, hipStream_t s) {
  T2P_REQUIRE(x && dy && dx && n > 0, "silu_backward arguments");
  hipLaunchKernelGGL(ew_kernel<1>, dim3(grid_for(n, 256)), dim3(256), 0, s, x, dy, dx, 0.f, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
int launch_axpy(float* y, const float* x, float a, long n, hipStream_t s) {
  T2P_REQUIRE(x && y && n > 0, "axpy arguments");
  hipLaunchKernelGGL(ew_kernel<2>, dim3(grid_for(n, 256)), dim3(256), 0, s, x, nullptr, y, a, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
int launch_add_scale(const float* a, const float* b, float alpha, float* out, long n, hipStream_t s) {
  T2P_REQUIRE(a && b && out && n > 0, "add_scale arguments");
  hipLaunchKernelGGL(ew_kernel<3>, dim3(grid_for(n, 256)), dim3(256), 0, s, a, b, out, alpha, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ src, const long ld_src, const long src_off, float* __restrict__ dst,
                                                        const long ld_dst, const long dst_off, const long rows, const int C, const int acc) {
  const long total = rows * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float v = src[r * ld_src + src_off + c];
    float* d = dst + r * ld_dst + dst_off + c;
    *d = acc ? *d + v : v;
  }
}
int launch_copy_cols(const float* src, long ld_src, long src_off, float* dst, long ld_dst, long dst_off, long rows, int C, int accumulate,
                     hipStream_t s) {
  T2P_REQUIRE(src && dst && rows > 0 && C > 0 && ld_src >= src_off + C && ld_dst >= dst_off + C, "copy_cols arguments");
  hipLaunchKernelGGL(copy_cols_kernel, dim3(grid_for(rows * C, 256)), dim3(256), 0, s, src, ld_src, src_off, dst, ld_dst, dst_off, rows, C, accumulate);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// out[z][n] += sum over the rows of chunk (blockIdx.y) of sample z:  64 columns x 4 row lanes per block
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ dy, const long rows_per_z, const int N, const long ld,
                                                     float* __restrict__ out, const long ld_out, const int rows_per_block) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl, z = blockIdx.z;
  const long r0 = (long)blockIdx.y * rows_per_block, r1 = min(rows_per_z, r0 + rows_per_block);
  float a = 0.f;
  if (n < N)
    for (long r = r0 + rl; r < r1; r += 4) a += dy[((long)z * rows_per_z + r) * ld + n];
  red[rl][cl] = a;
  __syncthreads();
  if (rl == 0 && n < N) unsafeAtomicAdd(out + (long)z * ld_out + n, red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl]);
}
// fixed-order form: the block sums of colsum_kernel go to ws [z][chunk][N], colsum_finish_kernel adds the chunks in order
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ dy, const long rows_per_z, const int N, const long ld,
                                                             float* __restrict__ ws, const int rows_per_block) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl, z = blockIdx.z;
  const long r0 = (long)blockIdx.y * rows_per_block, r1 = min(rows_per_z, r0 + rows_per_block);
  float a = 0.f;
  if (n < N)
    for (long r = r0 + rl; r < r1; r += 4) a += dy[((long)z * rows_per_z + r) * ld + n];
  red[rl][cl] = a;
  __syncthreads();
  if (rl == 0 && n < N) ws[((long)z * gridDim.y + blockIdx.y) * N + n] = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
}
// 64 columns x 4 row lanes per block: lane l adds chunks l, l + 4, ... in order, then the four lane sums are added in lane order
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ ws, const int nchunk, const int N, float* __restrict__ out,
                                                            const long ld_out, const int accumulate) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl, z = blockIdx.y;
  float a = 0.f;
  if (n < N)
    for (int k = rl; k < nchunk; k += 4) a += ws[((long)z * nchunk + k) * N + n];
  red[rl][cl] = a;
  __syncthreads();
  if (rl == 0 && n < N) {
    const float t = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
    float* o = out + (long)z * ld_out + n;
    *o = accumulate ? *o + t : t;
  }
}
long colsum_ws_floats(int nz, long rows_per_z, int N) { return (long)nz * cdiv_l(rows_per_z, 256) * N; }
int launch_colsum(const float* dy, int nz, long rows_per_z, int N, long ld, float* out, long ld_out, int accumulate, float* ws, hipStream_t s) {
  T2P_REQUIRE(dy && out && nz > 0 && nz <= 65535 && rows_per_z > 0 && N > 0 && ld >= N && ld_out >= N, "colsum arguments");
  const int rpb = 256, nchunk = cdiv_l(rows_per_z, rpb);
  T2P_REQUIRE(nchunk <= 65535, "colsum rows");
  if (!ws) {
    if (!accumulate) T2P_HIP_CHECK(hipMemset2DAsync(out, ld_out * sizeof(float), 0, N * sizeof(float), nz, s));
    hipLaunchKernelGGL(colsum_kernel, dim3(cdiv_l(N, 64), nchunk, nz), dim3(256), 0, s, dy, rows_per_z, N, ld, out, ld_out, rpb);
  } else {
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(cdiv_l(N, 64), nchunk, nz), dim3(256), 0, s, dy, rows_per_z, N, ld, ws, rpb);
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(cdiv_l(N, 64), nz), dim3(256), 0, s, (const float*)ws, nchunk, N, out, ld_out, accumulate);
  }
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- 2x nearest up-sampling / 2x2 mean down-sampling --------------------------------------------------------------------------------
template <int OP>   // 0 up, 1 up backward, 2 down, 3 down backward; (H, W) = the SMALL map of the pair
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ in, float* __restrict__ out, const int H, const int W, const int C,
                                                       const long total_small) {
  const int W2 = 2 * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total_small; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long t = i / C;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H);
    const long b = t / H;
    const long big = ((b * 2 * H + 2 * y) * W2 + 2 * x) * C + c;     // top-left of the 2x2 block in the large map
    const long o01 = C, o10 = (long)W2 * C, o11 = (long)W2 * C + C;
    if (OP == 0) { const float v = in[i]; out[big] = v; out[big + o01] = v; out[big + o10] = v; out[big + o11] = v; }
    if (OP == 1) out[i] += in[big] + in[big + o01] + in[big + o10] + in[big + o11];
    if (OP == 2) out[i] = 0.25f * (in[big] + in[big + o01] + in[big + o10] + in[big + o11]);
    if (OP == 3) { const float v = 0.25f * in[i]; out[big] += v; out[big + o01] += v; out[big + o10] += v; out[big + o11] += v; }
  }
}
#define T2P_RESAMPLE(name, OP, HS, WS)                                                                              \
  int name(const float* a, float* b, int B, int H, int W, int C, hipStream_t s) {                                   \
    T2P_REQUIRE(a && b && B > 0 && H > 0 && W > 0 && C > 0 && (HS) > 0 && (WS) > 0, #name " arguments");             \
    const long total = (long)B * (HS) * (WS) * C;                                                                   \
    hipLaunchKernelGGL(resample_kernel<OP>, dim3(grid_for(total, 256)), dim3(256), 0, s, a, b, (HS), (WS), C, total); \
    T2P_HIP_CHECK(hipGetLastError());                                                                               \
    return T2P_OK;                                                                                                  \
  }
T2P_RESAMPLE(launch_up2, 0, H, W)                   // x [B][H][W][C] -> y [B][2H][2W][C]
T2P_RESAMPLE(launch_up2_backward, 1, H, W)          // dy [B][2H][2W][C] -> dx [B][H][W][C] +=
int launch_down2(const float* x, float* y, int B, int H, int W, int C, hipStream_t s) {   // x [B][H][W][C] -> y [B][H/2][W/2][C]
  T2P_REQUIRE(x && y && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0, "down2 arguments");
  const long total = (long)B * (H / 2) * (W / 2) * C;
  hipLaunchKernelGGL(resample_kernel<2>, dim3(grid_for(total, 256)), dim3(256), 0, s, x, y, H / 2, W / 2, C, total);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
int launch_down2_backward(const float* dy, float* dx, int B, int H, int W, int C, hipStream_t s) {   // dy [B][H/2][W/2][C] -> dx [B][H][W][C] +=
  T2P_REQUIRE(dy && dx && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0, "down2_backward arguments");
  const long total = (long)B * (H / 2) * (W / 2) * C;
  hipLaunchKernelGGL(resample_kernel<3>, dim3(grid_for(total, 256)), dim3(256), 0, s, dy, dx, H / 2, W / 2, C, total);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- dropout -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const unsigned char* __restrict__ keep, const float inv_keep,
                                                      float* __restrict__ y, const long n, const int acc) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = keep[i] ? x[i] * inv_keep : 0.f;
    y[i] = acc ? y[i] + v : v;
  }
}
int launch_dropout(const float* x, const unsigned char* keep, float inv_keep, float* y, long n, int accumulate, hipStream_t s) {
  T2P_REQUIRE(x && keep && y && n > 0, "dropout arguments");
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, x, keep, inv_keep, y, n, accumulate);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* __restrict__ keep, const long n, const float p,
                                                           const unsigned long long seed, const unsigned long long stream_id) {
  const long nq = (n + 3) / 4;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    uint32_t w[4];
    philox_counter_training(w, q, stream_id);
    philox4x32_10(w, seed);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = q * 4 + j;
      if (i < n) keep[i] = philox_uniform24(w[j]) >= p ? 1 : 0;
    }
  }
}
int launch_dropout_mask(unsigned char* keep, long n, float p, unsigned long long seed, unsigned long long stream_id, hipStream_t s) {
  T2P_REQUIRE(keep && n > 0 && p >= 0.f && p < 1.f, "dropout_mask arguments");
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, keep, n, p, seed, stream_id);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- convolution weight layouts -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_w_prep_kernel(const float* __restrict__ w, float* __restrict__ wf, float* __restrict__ wd, const int Co,
                                                          const int Ci, const int Cip, const int Cop) {
  const long nf = (long)Co * 9 * Cip, nd = (long)Ci * 9 * Cop;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nf + nd; i += (long)gridDim.x * 256) {
    if (i < nf) {
      const int ci = (int)(i % Cip), t = (int)((i / Cip) % 9), co = (int)(i / ((long)Cip * 9));
      wf[i] = ci < Ci ? w[((long)co * Ci + ci) * 9 + t] : 0.f;
    } else if (wd) {
      const long j = i - nf;
      const int co = (int)(j % Cop), t = (int)((j / Cop) % 9), ci = (int)(j / ((long)Cop * 9));
      wd[j] = co < Co ? w[((long)co * Ci + ci) * 9 + (8 - t)] : 0.f;
    }
  }
}
int launch_conv_w_prep(const float* w, float* wf, float* wd, int Co, int Ci, int Cip, int Cop, hipStream_t s) {
  T2P_REQUIRE(w && wf && Co > 0 && Ci > 0 && Cip >= Ci && Cop >= Co, "conv_w_prep arguments");
  const long n = (long)Co * 9 * Cip + (wd ? (long)Ci * 9 * Cop : 0);
  hipLaunchKernelGGL(conv_w_prep_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, w, wf, wd, Co, Ci, Cip, Cop);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
__global__ __launch_bounds__(256) void conv_w_grad_fold_kernel(const float* __restrict__ dwc, float* __restrict__ gw, const int Co, const int Ci,
                                                               const int Cip) {
  const long n = (long)Co * Ci * 9;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int t = (int)(i % 9), ci = (int)((i / 9) % Ci), co = (int)(i / ((long)Ci * 9));
    gw[i] += dwc[((long)co * 9 + t) * Cip + ci];
  }
}
int launch_conv_w_grad_fold(const float* dwc, float* gw, int Co, int Ci, int Cip, hipStream_t s) {
  T2P_REQUIRE(dwc && gw && Co > 0 && Ci > 0 && Cip >= Ci, "conv_w_grad_fold arguments");
  hipLaunchKernelGGL(conv_w_grad_fold_kernel, dim3(grid_for((long)Co * Ci * 9, 256)), dim3(256), 0, s, dwc, gw, Co, Ci, Cip);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// =====================================================================================================================================
// denoising score matching (VE, VP and sub-VP SDEs)
// =====================================================================================================================================
// Not wave_reduce.h's block_sum<1, 4>: these add sh[0] + sh[1] + sh[2] + sh[3] without a leading zero (the sign of a -0 total differs)
// and put their second barrier after the read, so `sh` may be reused at once.
__device__ inline float block_sum_256(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return r;
}
__device__ inline double block_sum_256_d(double v, double* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return r;
}

// t[b]: given, or t = eps + (1 - eps) u with u from Philox keyed by (seed, step), counter = the sample (the same stream for every SDE)
__device__ inline float dsm_time(const float* __restrict__ t_in, const int b, const float t_eps, const unsigned long long seed,
                                 const unsigned long long step) {
  if (t_in) return t_in[b];
  uint32_t c[4];
  philox_counter_training(c, b, step);
  philox4x32_10(c, seed);
  return philox_uniform24(c[0]) * (1.f - t_eps) + t_eps;
}
__global__ void dsm_prepare_kernel(const float* __restrict__ t_in, const int B, const float t_eps, const float sigma_min, const float sigma_max,
                                   const int N, const float* __restrict__ inv_sigma_table, const unsigned long long seed,
                                   const unsigned long long step, float* __restrict__ t_out, float* __restrict__ stdv, int* __restrict__ labels,
                                   float* __restrict__ scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float t = dsm_time(t_in, b, t_eps, seed, step);
  t_out[b] = t;
  stdv[b] = sigma_min * powf(sigma_max / sigma_min, t);
  int lab = (int)rintf((1.f - t) * (float)(N - 1));
  lab = min(max(lab, 0), N - 1);
  labels[b] = lab;
  scale[b] = inv_sigma_table ? inv_sigma_table[lab] : 1.f;
}
int launch_dsm_prepare(const float* t_in, int B, float t_eps, float sigma_min, float sigma_max, int N, const float* inv_sigma_table,
                       unsigned long long seed, unsigned long long step, float* t_out, float* std, int* labels, float* scale, hipStream_t s) {
  T2P_REQUIRE(B > 0 && N >= 2 && t_out && std && labels && scale && sigma_min > 0.f && sigma_max > sigma_min, "dsm_prepare arguments");
  hipLaunchKernelGGL(dsm_prepare_kernel, dim3(cdiv_l(B, 64)), dim3(64), 0, s, t_in, B, t_eps, sigma_min, sigma_max, N, inv_sigma_table, seed, step,
                     t_out, std, labels, scale);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// VP (subvp == 0) and sub-VP (subvp == 1).  The exponent lmc is evaluated in double from the fp32 t and 1 - exp(2 lmc) as -expm1(2 lmc):
// the reference's fp32 1 - exp(.) cancels (quantised to 6e-8 / (1 - exp(2 lmc)) relative), this form does not, so the result is the more
// accurate one and never differs through a cancellation of its own.  The time label stays the reference's fp32 product (its integer part
// is a table index).
__global__ void dsm_prepare_vp_kernel(const float* __restrict__ t_in, const int B, const float t_eps, const double beta_min, const double beta_max,
                                      const int subvp, const int N, const float* __restrict__ std_table, const float* __restrict__ inv_sigma_table,
                                      const unsigned long long seed, const unsigned long long step, float* __restrict__ t_out,
                                      float* __restrict__ mean_coef, float* __restrict__ stdv, int* __restrict__ labels, float* __restrict__ labels_f,
                                      float* __restrict__ scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float t = dsm_time(t_in, b, t_eps, seed, step);
  t_out[b] = t;
  const double td = (double)t;
  const double lmc = -0.25 * td * td * (beta_max - beta_min) - 0.5 * td * beta_min;
  const double var = -expm1(2.0 * lmc);                        // 1 - exp(2 lmc)
  mean_coef[b] = (float)exp(lmc);
  stdv[b] = (float)(subvp ? var : sqrt(var));
  const float lf = t * (subvp ? 999.f : (float)(N - 1));
  int idx = (int)lf;                                            // labels.long(): truncation
  idx = min(max(idx, 0), N - 1);                              // clamped: labels[] is a safe TABLE index, not always trunc(labels_f) -- sub-VP
  labels_f[b] = lf;                                             // without a sigma table and N < 1000 has 999 t >= N (the index is unused there)
  labels[b] = idx;
  const double div = subvp ? var : (double)std_table[idx];      // the score's divisor: continuous (sub-VP) / the discrete table entry (VP)
  scale[b] = (float)(-(inv_sigma_table ? (double)inv_sigma_table[idx] : 1.0) / div);
}
int launch_dsm_prepare_vp(const float* t_in, int B, float t_eps, double beta_min, double beta_max, int subvp, int N, const float* std_table,
                          const float* inv_sigma_table, unsigned long long seed, unsigned long long step, float* t_out, float* mean_coef,
                          float* std, int* labels, float* labels_f, float* scale, hipStream_t s) {
  T2P_REQUIRE(B > 0 && N >= 2 && t_out && mean_coef && std && labels && labels_f && scale && beta_min > 0.0 && beta_max > beta_min,
              "dsm_prepare_vp arguments");
  T2P_REQUIRE(subvp ? (!inv_sigma_table || N >= 1000) : std_table != nullptr,
              "dsm_prepare_vp: VP needs the discrete std table; sub-VP with a sigma table needs N >= 1000 (its label is 999 t)");
  hipLaunchKernelGGL(dsm_prepare_vp_kernel, dim3(cdiv_l(B, 64)), dim3(64), 0, s, t_in, B, t_eps, beta_min, beta_max, subvp, N, std_table,
                     inv_sigma_table, seed, step, t_out, mean_coef, std, labels, labels_f, scale);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- secondary-structure block dropout (losses.py:54-64, called at :106-107) ---------------------------------------------------------------
// one workgroup per block (sample, start, end): rows[sample][r] = 1 for r in start .. min(end, L) when the block is dropped.  The decision is
// drop[n] when given, else u < p with u the Philox uniform dsm_time forms ((c0 >> 8) 2^-24), counter = the block index, key = seed.  Every
// writer writes 1 (plain byte stores); rows is zeroed by the launcher.  A block whose sample or start lies outside the table writes nothing
__global__ __launch_bounds__(64) void ss_block_rows_kernel(const int* __restrict__ blocks, const int n, const unsigned char* __restrict__ drop,
                                                           const float p, const unsigned long long seed, const unsigned long long stream_id,
                                                           const int B, const int L, unsigned char* __restrict__ rows,
                                                           unsigned char* __restrict__ drop_out) {
  const int k = blockIdx.x;
  if (k >= n) return;
  bool d;
  if (drop) {
    d = drop[k] != 0;
  } else {
    uint32_t c[4];
    philox_counter_training(c, k, stream_id);
    philox4x32_10(c, seed);
    d = philox_uniform24(c[0]) < p;
  }
  if (drop_out && threadIdx.x == 0) drop_out[k] = d ? 1 : 0;
  const int b = blocks[3 * k], start = blocks[3 * k + 1], end = min(blocks[3 * k + 2], L);
  if (!d || b < 0 || b >= B || start < 0) return;
  for (int r = start + (int)threadIdx.x; r < end; r += 64) rows[(long)b * L + r] = 1;
}
int launch_ss_block_rows(const int* blocks, int n, const unsigned char* drop, float p, unsigned long long seed, unsigned long long stream_id,
                         int B, int L, unsigned char* rows, unsigned char* drop_out, hipStream_t s) {
  T2P_REQUIRE(blocks && rows && n > 0 && B > 0 && L > 0 && p >= 0.f && p <= 1.f, "ss_block_rows arguments");
  T2P_HIP_CHECK(hipMemsetAsync(rows, 0, (size_t)B * L, s));
  hipLaunchKernelGGL(ss_block_rows_kernel, dim3(n), dim3(64), 0, s, blocks, n, drop, p, seed, stream_id, B, L, rows, drop_out);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- text-context dropout (training for classifier-free guidance: a dropped sample trains on context * 0) --------------------------------
// one thread per sample: drop[b] = u < p, u the Philox uniform dsm_time forms ((c0 >> 8) 2^-24), counter = the sample index, key = seed
__global__ __launch_bounds__(64) void context_drop_draw_kernel(const int B, const float p, const unsigned long long seed,
                                                               const unsigned long long stream_id, unsigned char* __restrict__ drop) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint32_t c[4];
  philox_counter_training(c, b, stream_id);
  philox4x32_10(c, seed);
  drop[b] = philox_uniform24(c[0]) < p ? 1 : 0;
}
int launch_context_drop_draw(int B, float p, unsigned long long seed, unsigned long long stream_id, unsigned char* drop, hipStream_t s) {
  T2P_REQUIRE(drop && B > 0 && p >= 0.f && p <= 1.f, "context_drop_draw arguments");
  hipLaunchKernelGGL(context_drop_draw_kernel, dim3(cdiv_l(B, 64)), dim3(64), 0, s, B, p, seed, stream_id, drop);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// grid (chunks of ZERO_ROW_CHUNK float4, B, 1 or 2 buffers): the workgroups of a kept sample read its flag and exit; those of a dropped
// one store +0.0f over their chunk of row b (16-byte stores; a store, not a product: Inf and NaN become 0 too)
constexpr int ZERO_ROW_CHUNK = 1024;               // float4 per workgroup: four stores per thread
__global__ __launch_bounds__(256) void zero_sample_rows_kernel(float4* __restrict__ x0, float4* __restrict__ x1, const long n4,
                                                               const unsigned char* __restrict__ drop) {
  const int b = blockIdx.y;
  if (!drop[b]) return;
  float4* __restrict__ row = (blockIdx.z ? x1 : x0) + (long)b * n4;
  const long begin = (long)blockIdx.x * ZERO_ROW_CHUNK;
  const long end = begin + ZERO_ROW_CHUNK < n4 ? begin + ZERO_ROW_CHUNK : n4;
  for (long i = begin + threadIdx.x; i < end; i += 256) row[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
int launch_zero_sample_rows(float* x0, float* x1, int B, long n, const unsigned char* drop, hipStream_t s) {
  T2P_REQUIRE(x0 && drop && B > 0 && B <= 65535 && n > 0, "zero_sample_rows arguments");
  T2P_REQUIRE(n % 4 == 0, "zero_sample_rows: the row length must be a multiple of 4 floats (16-byte stores)");
  T2P_REQUIRE(((uintptr_t)x0 & 15) == 0 && ((uintptr_t)x1 & 15) == 0, "zero_sample_rows: the buffers must be 16-byte aligned");
  const long n4 = n / 4, chunks = (n4 + ZERO_ROW_CHUNK - 1) / ZERO_ROW_CHUNK;
  T2P_REQUIRE(chunks < (1L << 31), "zero_sample_rows: row too long");
  hipLaunchKernelGGL(zero_sample_rows_kernel, dim3((unsigned)chunks, B, x1 ? 2 : 1), dim3(256), 0, s, reinterpret_cast<float4*>(x0),
                     reinterpret_cast<float4*>(x1), n4, drop);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- random inpainting mask (utils.py:15-60, called by train.py before every train and eval step) ----------------------------------------
// grid B, 256 threads: thread j is residue j of sample blockIdx.x (L <= 256).  Counter indices within the stream (training layout):
// 0 the mode (word 0); (b + 1) 2^32 sample b's count and window start (words 0, 1); (b + 1) 2^32 + 1 + j residue j's key (word 0).
// Random subset: residue j is masked iff fewer than r of the l keys sort before its own (ties to the lower index), counted from LDS --
// exactly r residues, every subset of that size equally likely.  PAIR4: L % 4 == 0 and pair 4-byte aligned, four pixels per store
template <bool PAIR4>
__global__ __launch_bounds__(256) void inpaint_mask_draw_kernel(const int* __restrict__ llh, const int L, const float p_random,
                                                                const float contig_above, const unsigned long long seed,
                                                                const unsigned long long stream_id, const int force_mode,
                                                                unsigned char* __restrict__ flags, unsigned char* __restrict__ pair,
                                                                int* __restrict__ mode_out) {
  __shared__ uint32_t keys[256];
  __shared__ __align__(4) unsigned char fl[256];
  const int b = blockIdx.x, j = threadIdx.x;
  int mode = force_mode;
  uint32_t c[4];
  if (mode < 0) {
    philox_counter_training(c, 0, stream_id);
    philox4x32_10(c, seed);
    const float u0 = philox_uniform24(c[0]);
    mode = u0 < p_random ? 1 : u0 > contig_above ? 2 : 0;
  }
  if (mode_out && b == 0 && j == 0) *mode_out = mode;
  const int l = llh[3 * b], lo = llh[3 * b + 1], hi = llh[3 * b + 2];
  const long base = (long)(b + 1) << 32;
  philox_counter_training(c, base, stream_id);
  philox4x32_10(c, seed);
  const int r = lo + (int)(((unsigned long long)(c[0] >> 8) * (unsigned long long)(hi - lo)) >> 24);
  const int start = (int)(((unsigned long long)(c[1] >> 8) * (unsigned long long)(l - r)) >> 24);
  uint32_t key = 0;
  if (mode == 1 && j < l) {
    philox_counter_training(c, base + 1 + j, stream_id);
    philox4x32_10(c, seed);
    key = c[0];
  }
  keys[j] = key;
  __syncthreads();
  bool f = mode == 0;
  if (mode == 2) f = j >= start && j < start + r;
  if (mode == 1 && j < l) {
    int rank = 0;
    for (int i = 0; i < l; ++i) {
      const uint32_t ki = keys[i];
      rank += (ki < key || (ki == key && i < j)) ? 1 : 0;
    }
    f = rank < r;
  }
  fl[j] = f ? 1 : 0;
  if (j < L) flags[(long)b * L + j] = f ? 1 : 0;
  __syncthreads();
  const int HW = L * L;
  if (PAIR4) {
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(pair + (long)b * HW);
    const uint32_t* fl4 = reinterpret_cast<const uint32_t*>(fl);
    for (int q = j; q < HW / 4; q += 256) {
      const int row = (4 * q) / L, col4 = (4 * q - row * L) >> 2;     // L % 4 == 0: the four pixels share a row
      out[q] = (fl[row] ? 0x01010101u : 0u) | fl4[col4];
    }
  } else {
    for (int p = j; p < HW; p += 256) {
      const int row = p / L;
      pair[(long)b * HW + p] = fl[row] | fl[p - row * L];
    }
  }
}
int launch_inpaint_mask_draw(const int* llh, int B, int L, float p_random, float contig_above, unsigned long long seed,
                             unsigned long long stream_id, int force_mode, unsigned char* flags, unsigned char* pair, int* mode_out,
                             hipStream_t s) {
  T2P_REQUIRE(llh && flags && pair && B > 0 && B <= 65535 && L > 0 && force_mode >= -1 && force_mode <= 2, "inpaint_mask_draw arguments");
  T2P_REQUIRE(L <= 256, "inpaint_mask_draw: one thread per residue, ranks counted in LDS: max_res_num <= 256");
  if (L % 4 == 0 && ((uintptr_t)pair & 3) == 0)
    hipLaunchKernelGGL(inpaint_mask_draw_kernel<true>, dim3(B), dim3(256), 0, s, llh, L, p_random, contig_above, seed, stream_id, force_mode, flags,
                       pair, mode_out);
  else
    hipLaunchKernelGGL(inpaint_mask_draw_kernel<false>, dim3(B), dim3(256), 0, s, llh, L, p_random, contig_above, seed, stream_id, force_mode, flags,
                       pair, mode_out);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// SS of dsm_perturb_kernel: the residue flags of the dropped blocks (SsRows), or none (NoSs: the kernel as it is without block dropout)
struct NoSs {};
struct SsRows { const unsigned char* rows; int L; };
// grid (chunks, B)
template <bool MEAN, class SS = NoSs>
__global__ __launch_bounds__(256) void dsm_perturb_kernel(const float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ stdv,
                                                          const float* __restrict__ mean_coef, const unsigned char* __restrict__ mask_pair,
                                                          const unsigned char* __restrict__ mask_inpaint, const int flags, const int C,
                                                          const int HW, float* __restrict__ perturbed, unsigned char* __restrict__ mask,
                                                          float* __restrict__ num_elem, const SS ss = SS()) {
  __shared__ float sh[4];
  const int b = blockIdx.y;
  const long per = (long)C * HW;
  const float sd = stdv[b];
  const float mc = MEAN ? mean_coef[b] : 1.f;
  float cnt = 0.f;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < per; j += (long)gridDim.x * 256) {
    const int c = (int)(j / HW), p = (int)(j - (long)c * HW);
    bool m = mask_pair[(long)b * HW + p] != 0;
    if ((flags & 1) && c == C - 1) m = false;
    if ((flags & 2) && c >= 4 && c < 7) m = false;
    if ((flags & 4) && !mask_inpaint[(long)b * HW + p]) m = false;
    const long i = (long)b * per + j;
    float xv = x[i];
    if constexpr (std::is_same<SS, SsRows>::value) {          // block_dropout: channels 4:7 on the rows and the columns of a dropped block
      if (c >= 4 && c < 7) {
        const int pi = p / ss.L, pj = p - pi * ss.L;
        if (ss.rows[(long)b * ss.L + pi] | ss.rows[(long)b * ss.L + pj]) xv = 0.f;
      }
    }
    if (MEAN) perturbed[i] = m ? mc * xv + sd * z[i] : xv;
    else perturbed[i] = m ? xv + sd * z[i] : xv;
    mask[i] = m ? 1 : 0;
    cnt += m ? 1.f : 0.f;
  }
  cnt = block_sum_256(cnt, sh);
  if (threadIdx.x == 0 && cnt != 0.f) unsafeAtomicAdd(num_elem + b, cnt);
}
int launch_dsm_perturb(const float* x, const float* z, const float* std, const float* mean_coef, const unsigned char* mask_pair,
                       const unsigned char* mask_inpaint, int cond_flags, int B, int C, int L, float* perturbed, unsigned char* mask,
                       float* num_elem, hipStream_t s, const unsigned char* ss_rows) {
  T2P_REQUIRE(x && z && std && mask_pair && perturbed && mask && num_elem && B > 0 && B <= 65535 && C > 0 && L > 0, "dsm_perturb arguments");
  T2P_REQUIRE(!(cond_flags & 4) || mask_inpaint, "dsm_perturb: the inpainting condition needs mask_inpaint");
  T2P_REQUIRE(!ss_rows || C >= 7, "dsm_perturb: block dropout needs the 8-channel layout (channels 4:7)");
  T2P_HIP_CHECK(hipMemsetAsync(num_elem, 0, B * sizeof(float), s));
  const long per = (long)C * L * L;
  const dim3 grid(std::min(64, cdiv_l(per, 256)), B);
  if (ss_rows) {
    const SsRows ss{ss_rows, L};
    if (mean_coef)
      hipLaunchKernelGGL((dsm_perturb_kernel<true, SsRows>), grid, dim3(256), 0, s, x, z, std, mean_coef, mask_pair, mask_inpaint, cond_flags, C,
                         L * L, perturbed, mask, num_elem, ss);
    else
      hipLaunchKernelGGL((dsm_perturb_kernel<false, SsRows>), grid, dim3(256), 0, s, x, z, std, mean_coef, mask_pair, mask_inpaint, cond_flags, C,
                         L * L, perturbed, mask, num_elem, ss);
  } else if (mean_coef)
    hipLaunchKernelGGL(dsm_perturb_kernel<true>, grid, dim3(256), 0, s, x, z, std, mean_coef, mask_pair, mask_inpaint, cond_flags, C, L * L, perturbed,
                       mask, num_elem);
  else
    hipLaunchKernelGGL(dsm_perturb_kernel<false>, grid, dim3(256), 0, s, x, z, std, mean_coef, mask_pair, mask_inpaint, cond_flags, C, L * L, perturbed,
                       mask, num_elem);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void dsm_loss_kernel(const float* __restrict__ o, const long ldo, const float* __restrict__ z,
                                                       const float* __restrict__ stdv, const float* __restrict__ scale,
                                                       const unsigned char* __restrict__ mask, const float* __restrict__ num_elem, const int B,
                                                       const int C, const int HW, double* __restrict__ loss_sum, float* __restrict__ d_o,
                                                       const long ld_do, float* __restrict__ score_nchw) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const long per = (long)C * HW;
  const float sd = stdv[b], is = scale[b];
  const float gscale = 2.f * sd * is / ((num_elem[b] + 1e-8f) * (float)B);
  double acc = 0.0;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < per; j += (long)gridDim.x * 256) {
    const int c = (int)(j / HW), p = (int)(j - (long)c * HW);
    const long i = (long)b * per + j;
    const float sc = o[((long)b * HW + p) * ldo + c] * is;
    if (score_nchw) score_nchw[i] = sc;
    const float r = sc * sd + z[i];
    const float m = mask[i] ? 1.f : 0.f;
    acc += (double)(r * r * m);
    if (d_o) d_o[((long)b * HW + p) * ld_do + c] = gscale * r * m;
  }
  acc = block_sum_256_d(acc, sh);
  if (threadIdx.x == 0) unsafeAtomicAdd(loss_sum + b, acc);
}
int launch_dsm_loss(const float* o, long ldo, const float* z, const float* std, const float* scale, const unsigned char* mask,
                    const float* num_elem, int B, int C, int L, double* loss_sum, float* d_o, long ld_do, float* score_nchw, hipStream_t s) {
  T2P_REQUIRE(o && z && std && scale && mask && num_elem && loss_sum && B > 0 && B <= 65535 && C > 0 && L > 0 && ldo >= C, "dsm_loss arguments");
  T2P_REQUIRE(!d_o || ld_do >= C, "dsm_loss: ld_do");
  T2P_HIP_CHECK(hipMemsetAsync(loss_sum, 0, B * sizeof(double), s));
  if (d_o && ld_do > C) T2P_HIP_CHECK(hipMemsetAsync(d_o, 0, (size_t)B * L * L * ld_do * sizeof(float), s));
  const long per = (long)C * L * L;
  hipLaunchKernelGGL(dsm_loss_kernel, dim3(std::min(64, cdiv_l(per, 256)), B), dim3(256), 0, s, o, ldo, z, std, scale, mask, num_elem, B, C, L * L,
                     loss_sum, d_o, ld_do, score_nchw);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
__global__ void dsm_finish_kernel(const double* __restrict__ loss_sum, const float* __restrict__ num_elem, const int B, float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double a = 0.0;
    for (int b = 0; b < B; ++b) a += loss_sum[b] / ((double)num_elem[b] + 1e-8);
    *loss = (float)(a / B);
  }
}
int launch_dsm_finish(const double* loss_sum, const float* num_elem, int B, float* loss, hipStream_t s) {
  T2P_REQUIRE(loss_sum && num_elem && loss && B > 0, "dsm_finish arguments");
  hipLaunchKernelGGL(dsm_finish_kernel, dim3(1), dim3(64), 0, s, loss_sum, num_elem, B, loss);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- the DDIM sampler's noise-prediction objective (sampler/diffusion_sampler.py:144-167) ----------------------------------------------
// torch.randint(0, T) of diffusion_sampler.py:166 from one 24-bit Philox word: ((w >> 8) T) >> 24 lies in [0, T) for every T <= 2^24
__device__ inline int ploss_draw_t(const int b, const int T, const unsigned long long seed, const unsigned long long stream_id) {
  uint32_t c[4];
  philox_counter_training(c, b, stream_id);
  philox4x32_10(c, seed);
  return (int)(((unsigned long long)(c[0] >> 8) * (unsigned long long)T) >> 24);
}
__global__ void ploss_prepare_kernel(const float* __restrict__ t_in, const int B, const int T, const float* __restrict__ sqrt_ac,
                                     const float* __restrict__ sqrt_1mac, const float* __restrict__ inv_sigma_table,
                                     const unsigned long long seed, const unsigned long long stream_id, float* __restrict__ t_out,
                                     float* __restrict__ mean_coef, float* __restrict__ stdv, int* __restrict__ labels,
                                     float* __restrict__ scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int t;
  if (t_in) {                                                   // clamped in float first: no conversion of a NaN or of a value past int
    const float tf = t_in[b];
    t = tf >= (float)(T - 1) ? T - 1 : tf > 0.f ? (int)tf : 0;
  } else {
    t = ploss_draw_t(b, T, seed, stream_id);
  }
  t = min(max(t, 0), T - 1);                                    // the table index: never out of bounds
  t_out[b] = (float)t;
  labels[b] = t;
  mean_coef[b] = sqrt_ac[t];
  stdv[b] = sqrt_1mac[t];
  scale[b] = inv_sigma_table ? inv_sigma_table[t] : 1.f;        // UNetModel.forward's own h / sigmas[t] (ncsnpp.py:259-261)
}
int launch_ploss_prepare(const float* t_in, int B, int T, const float* sqrt_ac, const float* sqrt_1mac, const float* inv_sigma_table, int N,
                         unsigned long long seed, unsigned long long stream_id, float* t_out, float* mean_coef, float* std, int* labels,
                         float* scale, hipStream_t s) {
  T2P_REQUIRE(B > 0 && T >= 1 && T <= (1 << 24) && sqrt_ac && sqrt_1mac && t_out && mean_coef && std && labels && scale, "ploss_prepare arguments");
  T2P_REQUIRE(!inv_sigma_table || T <= N, "ploss_prepare: with a sigma table every timestep indexes it, timesteps <= num_scales");
  hipLaunchKernelGGL(ploss_prepare_kernel, dim3(cdiv_l(B, 64)), dim3(64), 0, s, t_in, B, T, sqrt_ac, sqrt_1mac, inv_sigma_table, seed, stream_id,
                     t_out, mean_coef, std, labels, scale);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
__global__ void ploss_draw_t_kernel(const int B, const int T, const unsigned long long seed, const unsigned long long stream_id,
                                    int* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = ploss_draw_t(b, T, seed, stream_id);
}
int launch_ploss_draw_t(int B, int T, unsigned long long seed, unsigned long long stream_id, int* out, hipStream_t s) {
  T2P_REQUIRE(B > 0 && T >= 1 && T <= (1 << 24) && out, "ploss_draw_t arguments");
  hipLaunchKernelGGL(ploss_draw_t_kernel, dim3(cdiv_l(B, 64)), dim3(64), 0, s, B, T, seed, stream_id, out);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// grid (chunks, B), the geometry and the summation of dsm_loss_kernel
template <bool L1>
__global__ __launch_bounds__(256) void ploss_loss_kernel(const float* __restrict__ o, const long ldo, const float* __restrict__ z,
                                                         const float* __restrict__ scale, const unsigned char* __restrict__ mask, const float* __restrict__ num_elem, const int B,
                                                         const int C, const int HW, double* __restrict__ loss_sum, float* __restrict__ d_o,
                                                         const long ld_do, float* __restrict__ pred_nchw) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const long per = (long)C * HW;
  const float is = scale[b];
  const float gscale = (L1 ? 1.f : 2.f) * is / ((num_elem[b] + 1e-8f) * (float)B);
  double acc = 0.0;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < per; j += (long)gridDim.x * 256) {
    const int c = (int)(j / HW), p = (int)(j - (long)c * HW);
    const long i = (long)b * per + j;
    const float ov = o[((long)b * HW + p) * ldo + c] * is;
    if (pred_nchw) pred_nchw[i] = ov;
    const float r = ov - z[i];
    const float m = mask[i] ? 1.f : 0.f;
    acc += (double)((L1 ? fabsf(r) : r * r) * m);
    if (d_o) {
      const float dr = L1 ? (r > 0.f ? 1.f : r < 0.f ? -1.f : 0.f) : r;      // torch.sign: 0 at 0 (and at NaN, where the loss says so)
      d_o[((long)b * HW + p) * ld_do + c] = gscale * dr * m;
    }
  }
  acc = block_sum_256_d(acc, sh);
  if (threadIdx.x == 0) unsafeAtomicAdd(loss_sum + b, acc);
}
int launch_ploss_loss(int l1, const float* o, long ldo, const float* z, const float* scale, const unsigned char* mask, const float* num_elem,
                      int B, int C, int L, double* loss_sum, float* d_o, long ld_do, float* pred_nchw, hipStream_t s) {
  T2P_REQUIRE(o && z && scale && mask && num_elem && loss_sum && B > 0 && B <= 65535 && C > 0 && L > 0 && ldo >= C, "ploss_loss arguments");
  T2P_REQUIRE(!d_o || ld_do >= C, "ploss_loss: ld_do");
  T2P_HIP_CHECK(hipMemsetAsync(loss_sum, 0, B * sizeof(double), s));
  if (d_o && ld_do > C) T2P_HIP_CHECK(hipMemsetAsync(d_o, 0, (size_t)B * L * L * ld_do * sizeof(float), s));
  const long per = (long)C * L * L;
  const dim3 grid(std::min(64, cdiv_l(per, 256)), B);
  if (l1)
    hipLaunchKernelGGL(ploss_loss_kernel<true>, grid, dim3(256), 0, s, o, ldo, z, scale, mask, num_elem, B, C, L * L, loss_sum, d_o, ld_do, pred_nchw);
  else
    hipLaunchKernelGGL(ploss_loss_kernel<false>, grid, dim3(256), 0, s, o, ldo, z, scale, mask, num_elem, B, C, L * L, loss_sum, d_o, ld_do, pred_nchw);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// =====================================================================================================================================
// optimizer and EMA
// =====================================================================================================================================
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, const long n, double* __restrict__ out) {
  __shared__ double sh[4];
  double a = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) { const float v = g[i]; a += (double)v * v; }
  a = block_sum_256_d(a, sh);
  if (threadIdx.x == 0) unsafeAtomicAdd(out, a);
}
// fixed order: one partial per block (SUMSQ_BLOCKS of them), then one block adds the partials
constexpr int SUMSQ_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, const long n, double* __restrict__ partial) {
  __shared__ double sh[4];
  double a = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) { const float v = g[i]; a += (double)v * v; }
  a = block_sum_256_d(a, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void sumsq_finish_kernel(const double* __restrict__ partial, const int np, double* __restrict__ out) {
  __shared__ double sh[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) a += partial[i];
  a = block_sum_256_d(a, sh);
  if (threadIdx.x == 0) *out = a;
}
int launch_sumsq(const float* g, long n, double* partial, double* out, hipStream_t s) {
  T2P_REQUIRE(g && out && n > 0, "sumsq arguments");
  const int nb = grid_for(n, 256, SUMSQ_BLOCKS);
  if (!partial) {
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, s, g, n, out);
  } else {
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, g, n, partial);
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, nb, out);
  }
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void adam_kernel(const AdamArgs a) {
  float clip = 1.f;
  if (a.grad_clip >= 0.f) clip = fminf(1.f, a.grad_clip / ((float)sqrt(*a.sumsq) + 1e-6f));
  const float step = a.lr / a.bias1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
    float g = a.g[i] * clip;
    a.g[i] = g;                                        // clip_grad_norm_ scales .grad in place
    if (a.weight_decay != 0.f) g += a.weight_decay * a.p[i];
    const float m = a.beta1 * a.m[i] + a.one_minus_beta1 * g;
    const float v = a.beta2 * a.v[i] + a.one_minus_beta2 * g * g;
    a.m[i] = m; a.v[i] = v;
    a.p[i] -= step * m / (sqrtf(v) / a.bias2_sqrt + a.eps);
  }
}
int launch_adam(const AdamArgs& a, hipStream_t s) {
  T2P_REQUIRE(a.p && a.g && a.m && a.v && a.n > 0 && a.bias1 > 0.f && a.bias2_sqrt > 0.f, "adam arguments");
  T2P_REQUIRE(a.grad_clip < 0.f || a.sumsq, "adam: clipping needs the gradient's sum of squares");
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(a.n, 256, 4096)), dim3(256), 0, s, a);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ shadow, const float* __restrict__ p, const float omd, const long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) { const float sv = shadow[i]; shadow[i] = sv - omd * (sv - p[i]); }
}
int launch_ema(float* shadow, const float* p, float one_minus_decay, long n, hipStream_t s) {
  T2P_REQUIRE(shadow && p && n > 0, "ema arguments");
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, shadow, p, one_minus_decay, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, const float a, const long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] *= a;
}
int launch_scale(float* x, float a, long n, hipStream_t s) {
  T2P_REQUIRE(x && n > 0, "scale arguments");
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, x, a, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// ---- power-of-two seed scale chosen from the seed itself (16-bit VP / sub-VP step) --------------------------------------------------------
// |x| of a finite non-negative float orders as its bit pattern, so an integer atomicMax gives max |x| independent of the order of arrival
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, const long n, unsigned int* __restrict__ out) {
  unsigned int m = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = max(m, __float_as_uint(fabsf(x[i])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(out, m);
}
// v > 0 finite = (1 + frac 2^-23) 2^e: returns frac (23 bits) and e, a subnormal v normalised first
__device__ inline unsigned int pow2_split(const float v, int* e) {
  const unsigned int b = __float_as_uint(v);
  int ex = (int)(b >> 23);
  unsigned int frac = b & 0x7fffffu;
  if (ex == 0) {                                   // subnormal: frac != 0, its leading one moves up to the implicit position
    const int sh = __clz((int)frac) - 8;
    frac = (frac << sh) & 0x7fffffu;
    ex = 1 - sh;
  }
  *e = ex - 127;
  return frac;
}
__global__ void seed_scale_kernel(const unsigned int* __restrict__ absmax, const float target, float* __restrict__ s2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float m = __uint_as_float(*absmax);
  float S = 1.f;
  if (m > 0.f && m < INFINITY) {                 // (a NaN or infinite seed keeps S = 1: the loss is not finite and apply() refuses)
    // m = fm 2^em, target = ft 2^et, fm and ft in [1, 2): floor(log2(target / m)) = et - em - (ft < fm).  From the bit patterns, not from
    // the quotient: target / m overflows for a subnormal m, and frexpf of an infinity leaves the exponent unspecified
    int em = 0, et = 0;
    const unsigned int fm = pow2_split(m, &em), ft = pow2_split(target, &et);
    S = ldexpf(1.f, min(max(et - em - (ft < fm ? 1 : 0), -60), 60));
  }
  s2[0] = S; s2[1] = 1.f / S;
}
__global__ __launch_bounds__(256) void scale_dev_kernel(float* __restrict__ x, const float* __restrict__ a, const long n) {
  const float av = *a;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] *= av;
}
int launch_seed_scale(const float* x, long n, float target, unsigned int* absmax, float* s2, hipStream_t s) {
  T2P_REQUIRE(x && n > 0 && absmax && s2 && target > 0.f, "seed_scale arguments");
  T2P_HIP_CHECK(hipMemsetAsync(absmax, 0, sizeof(unsigned int), s));
  hipLaunchKernelGGL(absmax_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, x, n, absmax);
  hipLaunchKernelGGL(seed_scale_kernel, dim3(1), dim3(64), 0, s, absmax, target, s2);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}
int launch_scale_dev(float* x, const float* a, long n, hipStream_t s) {
  T2P_REQUIRE(x && a && n > 0, "scale_dev arguments");
  hipLaunchKernelGGL(scale_dev_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, x, a, n);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

}  // namespace t2p
