// Row-resident GEMM for the K = 512 projections of the SpatialTransformer (gfx950): C = alpha (A W^T + bias_n + R), or the fused
// GEGLU form, with 16-bit A, W and C.
//
// The 256 x 256 LDS-DMA kernel (gemm_dma.hip) has 8 K-tiles at K = 512: set-up, the first stage and the epilogue are half of a tile's
// time, one workgroup owns the CU, and a barrier in every K-tile keeps its waves in step, so nothing hides them.  Here
//   * a workgroup of 8 wavefronts owns 128 rows and brings all 128 x 512 activations into LDS once (128 KiB, LDS-DMA, the K-tile
//     image and chunk swizzle of gemm_dma_body); LDS holds nothing else;
//   * wavefront w owns the 64-column slices w, w + 8, ... over all 128 rows (the 128 x 64 wave tile, 128 accumulator registers, of
//     the 16x16x32 loop in gemm_dma.hip) and streams its own weight fragments L2 -> registers, two K-tiles ahead, from a
//     fragment-major copy of the weights (rowres_pack_kernel, weightpack.hip: the four fragments of a 32-deep step are 4 KiB
//     contiguous);
//   * only a wave's first slice synchronises, once per K-tile, so that its MFMAs start while later K-tiles of A are still
//     landing; after that the loop has no workgroup barrier and the waves drift apart: one wave's epilogue and first-fragment
//     latency sit under the MFMAs of the wave it shares a SIMD with.
// Same MFMA, same assignment of k to fragment positions, same K order (K-tile 0..7, step 0, 1) and the epilogue arithmetic of
// reg_epilogue: the results are bit-identical to the 256 x 256 kernel's.
#include <string>
#include <type_traits>

#include "gemm_mfma.h"
#include "t2p_kernels.h"

namespace t2p {

long g_rowres_launches = 0; // launches of the kernel since the library was loaded (tests: which plan a launch took)

bool gemm_rowres_eligible(const GemmParams& p) {
  if (p.dtype != DT_F16 && p.dtype != DT_BF16) return false;
  if (p.a_f32 || p.c_f32 || p.taps != 1 || p.C0 != 512 || p.A1 || p.C1 || p.a_up) return false;
  if (p.nz0 * p.nz1 != 1 || p.M % 128 != 0 || p.N % 64 != 0) return false;
  if (p.c_frag || p.col_stats || p.gn_out || p.bias_m || p.bias_bn || p.r_up || p.c_nchw || p.X0 || p.an_stats) return false;
  if (p.R && !p.r_lowp) return false;                            // the residual of these products is the 16-bit stream
  if (p.geglu && p.R) return false;
  // 16-byte row segments and 32-bit byte offsets, as reg_epilogue_ok asks
  if (p.lda0 % 8 != 0 || (p.geglu ? p.ldc % 4 != 0 : p.ldc % 8 != 0) || (p.R && p.ldr % 8 != 0)) return false;
  const long lim = (1L << 31) - 64;
  const long c_cols = p.geglu ? p.N / 2 : p.N;
  if ((long)p.M * p.lda0 * 2 >= lim || ((long)(p.M - 1) * p.ldc + c_cols) * 2 >= lim || (p.R && ((long)(p.M - 1) * p.ldr + p.N) * 2 >= lim)) return false;
  if ((long)p.N * 1024 >= lim) return false;
  return true;
}

#define T2P_RR_RD4(F, ADDR, I0)                                                                     \
  lds_read_b128_2k<I0>(F[0], ADDR); lds_read_b128_2k<I0 + 1>(F[1], ADDR);                            \
  lds_read_b128_2k<I0 + 2>(F[2], ADDR); lds_read_b128_2k<I0 + 3>(F[3], ADDR);
#define T2P_RR_W4(N, X)                                                                             \
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]) : "n"(N));
#define T2P_RR_M16(A, B, I0)                                                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j)       \
      Mma16<TC>::run(B[j], A[i], acc[I0 + i][j]);

template <typename TC>
__global__ __launch_bounds__(512) void gemm_rowres_kernel(const GemmParams p) {
  constexpr int NKT = 8;                                 // K-tiles of 64: K = 512
  constexpr int ASTAGE = 128 * 128;                      // one K-tile of the 128 rows
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 128;
  const int nslices = p.N >> 6;

  // ---- activations: 16 LDS-DMA instructions per K-tile (8 rows x 128 B each), two per wave --------------------------------------
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A0, (int)((((long)p.M - 1) * p.lda0 + 512) * 2));
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned a_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (wave * 2 + j) * 8 + prow;            // row of the tile; LDS position ppos of row r holds chunk ppos ^ ((r >> 1) & 7)
    a_off[j] = (unsigned)(m0 + r) * (unsigned)(p.lda0 * 2) + (unsigned)((ppos ^ ((r >> 1) & 7)) * 16);
  }
  auto issue_a = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned char* dst = smem + kt * ASTAGE + (wave * 2 + j) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, T2P_LDS_PTR(dst), 16, a_off[j] + (unsigned)(kt * 128), 0, 0, 0);
    }
  };

  // ---- weights: fragment-major, [slice][32-deep step 0..15][column tile 0..3][lane] x 16 bytes -----------------------------------
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(p.Bw_rf, (int)((long)p.N * 1024));
  const unsigned b_lane = (unsigned)lane * 16u;
  u32x4_t Bf[2][2][4];                                   // [ring slot = K-tile & 1][step][column tile]
  auto load_b = [&](auto SLOT, int slice, int kt) __attribute__((always_inline)) {
    constexpr int slot = decltype(SLOT)::value;
    // a wave without a slice (N < 512) takes the same path with every load out of range: zeros, and the same vmcnt accounting
    // (in the per-lane offset: the range check of a raw buffer covers that one, not the scalar offset)
    const unsigned vo = slice < nslices ? b_lane + (unsigned)((slice * 16 + kt * 2) * 4096) : DMA_OOB;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) Bf[slot][ks][j] = __builtin_amdgcn_raw_buffer_load_b128(rB, vo + (unsigned)(ks * 4096 + j * 1024), 0, 0);
  };

  // A fragment of 16-row tile i, step ks of K-tile kt: lane (r = lane & 15, g = lane >> 4) reads logical chunk 4 ks + g of row
  // 16 i + r; the swizzle term depends on r only, so tile i is the immediate offset i * 2048
  const unsigned lds_base = (unsigned)(unsigned long long)T2P_LDS_PTR(smem);
  unsigned a16[2];
  {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a16[ks] = lds_base + (unsigned)(r * 128 + (((4 * ks + g) ^ ((r >> 1) & 7)) << 4));
  }

  f32x4_t acc[8][4];
  // one K-tile of the wave tile: the MFMA order of the 16x16x32 loop in gemm_dma_body (weights first: transposed accumulators)
  auto ktile = [&](auto SLOT, int kt) __attribute__((always_inline)) {
    constexpr int slot = decltype(SLOT)::value;
    u32x4_t AL[4], AH[4];
    const unsigned aa0 = a16[0] + (unsigned)(kt * ASTAGE), aa1 = a16[1] + (unsigned)(kt * ASTAGE);
    T2P_RR_RD4(AL, aa0, 0)
    T2P_RR_RD4(AH, aa0, 4)
    T2P_RR_W4(4, AL)
    T2P_RR_M16(AL, Bf[slot][0], 0)
    T2P_RR_RD4(AL, aa1, 0)
    T2P_RR_W4(4, AH)
    T2P_RR_M16(AH, Bf[slot][0], 4)
    T2P_RR_RD4(AH, aa1, 4)
    T2P_RR_W4(4, AL)
    T2P_RR_M16(AL, Bf[slot][1], 0)
    T2P_RR_W4(0, AH)
    T2P_RR_M16(AH, Bf[slot][1], 4)
  };

  // ---- epilogue of one slice (reg_epilogue's arithmetic): lane (m = lane & 15, g = lane >> 4) holds, per 16-row tile, channels
  // [col0, col0 + 8) and [col0 + 32, col0 + 40) of row m, col0 = 64 slice + 8 g ------------------------------------------------
  const long c_cols = p.geglu ? p.N / 2 : p.N;
  const __amdgpu_buffer_rsrc_t rC = make_rsrc(p.C, (int)((((long)p.M - 1) * p.ldc + c_cols) * 2));
  const __amdgpu_buffer_rsrc_t rR = make_rsrc(p.R ? (const void*)p.R : (const void*)p.C, p.R ? (int)((((long)p.M - 1) * p.ldr + p.N) * 2) : 0);
  const bool has_r = p.R != nullptr, geglu = p.geglu != 0;
  const float alpha = p.alpha;
  const unsigned ldc_e = (unsigned)p.ldc, ldr_e = (unsigned)p.ldr;
  auto epilogue = [&](int slice) __attribute__((always_inline)) {
    int tx = threadIdx.x;
    asm volatile("" : "+v"(tx));       // nothing lane-derived of the epilogue is computed before the K loop and kept across it (registers)
    const int l16 = tx & 15, g4 = (tx & 63) >> 4;
    const int col0 = slice * 64 + 8 * g4;
    float bs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) bs[k] = 0.f;
    if (p.bias_n) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float4 t = *(const float4*)(p.bias_n + col0 + 32 * h + 4 * q);
          const int k = 8 * h + 4 * q;
          bs[k] = t.x; bs[k + 1] = t.y; bs[k + 2] = t.z; bs[k + 3] = t.w;
        }
    }
    float bm = 0.f;                                      // the general form adds (row bias + column bias): a real 0 + b (signed zeros)
    asm volatile("" : "+v"(bm));
    auto half = [&](auto HC) __attribute__((always_inline)) {
      constexpr int i0 = 4 * decltype(HC)::value;
      u32x4_t rr[4][2];
      if (has_r) {                                       // every element is read before the same lane writes it (R may be C)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            rr[i][h] = __builtin_amdgcn_raw_buffer_load_b128(rR, ((unsigned)(m0 + 16 * (i0 + i) + l16) * ldr_e + (unsigned)(col0 + 32 * h)) * 2u, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned row = (unsigned)(m0 + 16 * (i0 + i) + l16);
        float v[16];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * j + e] = acc[i0 + i][j][e];   // v[k]: channel col0 + (k & 7) + 32 (k >> 3)
        if (geglu) {
#pragma unroll
          for (int k = 0; k < 16; ++k) v[k] += bm + bs[k];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float* w = v + 8 * h;
            __builtin_amdgcn_raw_buffer_store_b64((u32x2_t){pack2<TC>(w[0] * gelu_erf_fast(w[1]), w[2] * gelu_erf_fast(w[3])),
                                                             pack2<TC>(w[4] * gelu_erf_fast(w[5]), w[6] * gelu_erf_fast(w[7]))},
                                                  rC, (row * ldc_e + (unsigned)((col0 + 32 * h) >> 1)) * 2u, 0, 0);
          }
          continue;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] += bs[k];
        if (has_r) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f32x4_res_t a = unpack4<TC>((u32x2_res_t){rr[i][h][0], rr[i][h][1]}), b = unpack4<TC>((u32x2_res_t){rr[i][h][2], rr[i][h][3]});
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[8 * h + e] += a[e]; v[8 * h + 4 + e] += b[e]; }
          }
        }
        if (alpha != 1.0f) {                             // (x * 1 = x exactly)
#pragma unroll
          for (int k = 0; k < 16; ++k) v[k] *= alpha;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float* w = v + 8 * h;
          const u32x4_t packed = {pack2<TC>(w[0], w[1]), pack2<TC>(w[2], w[3]), pack2<TC>(w[4], w[5]), pack2<TC>(w[6], w[7])};
          __builtin_amdgcn_raw_buffer_store_b128(packed, rC, (row * ldc_e + (unsigned)(col0 + 32 * h)) * 2u, 0, 0);
        }
      }
    };
    half(std::integral_constant<int, 0>{});
    half(std::integral_constant<int, 1>{});
  };
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  };
  using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;

  // ---- first slice: the activations land while it runs.  Issue order of a wave (vmcnt counts in order):
  //   A0 A1 B0 | A2 B1 | A3 B2 | ... | A7 B6 | B7       (A: 2 instructions, B: 8)
  // so when K-tile kt starts, everything up to B(kt) has landed once at most A(kt + 2) and B(kt + 1) are outstanding; the barrier
  // then says the same of every wave's part of A(kt).
  zero_acc();
  issue_a(0); issue_a(1);
  load_b(S0{}, wave, 0);
  issue_a(2);
  load_b(S1{}, wave, 1);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    if (kt <= 5) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if (kt == 6) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt & 1) ktile(S1{}, kt); else ktile(S0{}, kt);
    if (kt + 3 < NKT) issue_a(kt + 3);
    if (kt + 2 < NKT) { if (kt & 1) load_b(S1{}, wave, kt + 2); else load_b(S0{}, wave, kt + 2); }
  }
  if (wave < nslices) epilogue(wave);

  // ---- the wave's other slices: no barrier, weights two K-tiles ahead -----------------------------------------------------------
  for (int slice = wave + 8; slice < nslices; slice += 8) {
    zero_acc();
    load_b(S0{}, slice, 0);
    load_b(S1{}, slice, 1);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt & 1) ktile(S1{}, kt); else ktile(S0{}, kt);
      if (kt + 2 < NKT) { if (kt & 1) load_b(S1{}, slice, kt + 2); else load_b(S0{}, slice, kt + 2); }
    }
    epilogue(slice);
  }
}
#undef T2P_RR_RD4
#undef T2P_RR_W4
#undef T2P_RR_M16

template <typename TC>
static int launch_rowres_t(const GemmParams& p, hipStream_t stream) {
  constexpr int smem = 8 * 128 * 128;
  auto kern = gemm_rowres_kernel<TC>;
  T2P_TRY(ensure_dynamic_lds((const void*)kern, smem));
  hipLaunchKernelGGL(kern, dim3(p.M / 128), dim3(512), smem, stream, p);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

const char* gemm_rowres_kernel_name(int dtype) { return dtype == DT_F16 ? "gemm_rowres_kernel<f16_t>" : "gemm_rowres_kernel<bf16_t>"; }

int launch_gemm_rowres(const GemmParams& p, hipStream_t stream) {
  T2P_REQUIRE(gemm_rowres_eligible(p) && p.Bw_rf, "row-resident GEMM: not eligible (ask gemm_rowres_eligible) or no fragment-major weights");
  T2P_REQUIRE(((uintptr_t)p.A0 % 16) == 0 && ((uintptr_t)p.Bw_rf % 16) == 0 && ((uintptr_t)p.C % 16) == 0 && ((uintptr_t)p.R % 16) == 0 &&
              ((uintptr_t)p.bias_n % 16) == 0, "row-resident GEMM: operands must be 16-byte aligned");
  ++g_rowres_launches;
  return p.dtype == DT_BF16 ? launch_rowres_t<bf16_t>(p, stream) : launch_rowres_t<f16_t>(p, stream);
}

}  // namespace t2p
