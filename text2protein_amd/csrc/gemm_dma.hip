// LDS-DMA GEMM / implicit-GEMM 3x3 convolution kernels for gfx950 and their launchers: gemm_dma_kernel, gemm_dma_cfrag_kernel and the
// dx-shared-stage gemm_dxs_kernel (v1 in the text below is the register-staged gemm_kernel of gemm.hip).
#include <string>
#include <type_traits>

#include "gemm_device.h"
#include "launch_prof.h"

namespace t2p {

// =================================================================================================
// v2: LDS-DMA pipeline for 16-bit operands (the dominant kernel: 3x3 convolutions and large GEMMs).
//
// v1 above stages operands through registers; its ds_write_b128 traffic (~79 B/clk/CU) plus the
// fragment reads make it LDS-bound at about 15 % of the 16-bit MFMA peak.  Here both operand
// tiles go HBM/L2 -> LDS directly with `buffer_load_dwordx4 ... lds` (no VGPR round trip, no
// ds_write), which also gives the convolution's zero padding and all ragged edges for free: a
// lane whose source is outside the map / matrix gets an out-of-range buffer offset and the
// hardware writes zeros.
//   * workgroup = 8 wavefronts (4 x 2), tile BM x BN = 256 x 128, BK = 64 (128-byte LDS rows)
//   * LDS ring of 3 stages (3 x 48 KiB); the loads of K-tile t+2 are issued while tile t is being
//     multiplied; a counted `s_waitcnt vmcnt(6)` + one raw s_barrier per K-tile
//   * LDS image is lane-linear per DMA instruction (8 rows x 128 B), so the bank-conflict swizzle
//     is applied to the SOURCE chunk: position p of row r holds chunk p ^ ((r >> 1) & 7), and the
//     ds_read_b128 fragment reads apply the same XOR (conflict-free for all 16-lane groups)
//   * tile ids are remapped so that consecutive tiles (same A rows, neighbouring pixels) run on
//     the same XCD and share its L2
// Requirements (else v1 runs): 16-bit compute dtype, A in the compute dtype, C0 % 64 == 0 and
// C1 % 64 == 0, M >= 256, N >= 64, every operand smaller than 2 GiB.


// MODE 0: plain GEMM rows; 1: 3x3 convolution; 2: 3x3 convolution reading a half-resolution source
//
// Geometries (BM x BN block, WM x WN wavefronts, NST ring stages):
//   256 x 128, 4 x 2 waves (64 x 64 each),  3 stages (144 KiB): loads two K-tiles ahead
//   256 x 256, 2 x 4 waves (128 x 64 each), 2 stages (128 KiB): A fetched once for N = 256,
//       0.75 fragment reads per MFMA, half the barriers per FLOP
//   128 x 128, 2 x 2 waves (64 x 64 each),  2 stages ( 64 KiB): two workgroups per CU (short problems)
template <int I> __device__ inline void lds_read_b128(u32x4_t& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(I * 4096));
}

__device__ inline bool g_stagger_dbg(int dbg) { return (dbg & 128) == 0; }   // debug bit 128 turns the stagger off
template <int I> __device__ inline void lds_read_b128_1k(u32x4_t& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(I * 1024));
}

// Read-back half of the lean epilogue for one 64 x 64 slab, specialised at compile time so that the
// loop is branch-free: 8 LDS reads and (HAS_R) 8 residual loads at a time are in flight before the
// first use.  OUT: 0 fp32, 1 compute dtype, 2 GEGLU (interleaved value / gate columns ->
// compute dtype), 3 raw split-K partial.  Every variant issues exactly 16 stores.
// residual stored at half resolution (up-sampling blocks): row (b, y, x) reads residual row (b, y / 2, x / 2)
struct LeanRup { int on, W, HW, b_first, b_edge, hw4, w2; unsigned row_bytes, col_bytes; };

template <typename TC, int OUT, bool HAS_R, bool STATS, bool RL = false>
__device__ __forceinline__ void lean_slab(const float* sp, const __amdgpu_buffer_rsrc_t rC, const __amdgpu_buffer_rsrc_t rR,
                                          unsigned voc, const unsigned stc, unsigned vor, const unsigned str,
                                          const float4 bn0, const float4 bn1, const int row_first, const int b_edge,
                                          const float alpha, float* stats_dst, const LeanRup rup) {
  if constexpr (OUT == 3) {
#pragma unroll
    for (int h8 = 0; h8 < 2; ++h8) {
      f32x4_t v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = *(const f32x4_t*)(sp + (h8 * 8 + i) * 256);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v[i]), rC, voc, 0, 0);
        voc += stc;
      }
    }
    return;
  }
  float cs0 = 0.f, cs1 = 0.f, cs2 = 0.f, cs3 = 0.f, cq0 = 0.f, cq1 = 0.f, cq2 = 0.f, cq3 = 0.f;
#pragma unroll
  for (int h8 = 0; h8 < 2; ++h8) {
    f32x4_t v[8], rv[8];
    if constexpr (!HAS_R) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = *(const f32x4_t*)(sp + (h8 * 8 + i) * 256);
    }
    if constexpr (HAS_R) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        unsigned off = vor;
        if (rup.on) {                                  // wave-uniform; a tile spans at most two samples
          const int row = row_first + 4 * (h8 * 8 + i);
          const int bidx = rup.b_first + (row >= rup.b_edge ? 1 : 0);
          const int rem = row - bidx * rup.HW;
          const int y = rem / rup.W, x = rem - y * rup.W;
          off = vor == DMA_OOB ? DMA_OOB : (unsigned)(bidx * rup.hw4 + (y >> 1) * rup.w2 + (x >> 1)) * rup.row_bytes + rup.col_bytes;
        }
        if constexpr (RL) rv[i] = unpack4<TC>(__builtin_amdgcn_raw_buffer_load_b64(rR, off, 0, 0));   // 16-bit residual
        else rv[i] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rR, off, 0, 0));
        if (!rup.on) vor += str;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int it = h8 * 8 + i;
      if constexpr (HAS_R) {                          // 8 residual rows in flight, LDS reads 4 at a time (register budget)
        if (i % 4 == 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[i + k] = *(const f32x4_t*)(sp + (it + k) * 256);
        }
      }
      const bool second = row_first + 4 * it >= b_edge;
      float a0 = v[i][0] + (second ? bn1.x : bn0.x), a1 = v[i][1] + (second ? bn1.y : bn0.y);
      float a2 = v[i][2] + (second ? bn1.z : bn0.z), a3 = v[i][3] + (second ? bn1.w : bn0.w);
      if constexpr (HAS_R) { a0 += rv[i][0]; a1 += rv[i][1]; a2 += rv[i][2]; a3 += rv[i][3]; }
      if constexpr (OUT == 2) {
        // columns are interleaved (value_j, gate_j): out[row][col / 2 + {0, 1}] = value * gelu_erf(gate)
        // (GEGLU.forward, reference model/attention.py:42-44), stored in the compute dtype
        __builtin_amdgcn_raw_buffer_store_b32(pack2<TC>(a0 * gelu_erf_fast(a1), a2 * gelu_erf_fast(a3)), rC, voc, 0, 0);
      } else {
        a0 *= alpha; a1 *= alpha; a2 *= alpha; a3 *= alpha;
        if constexpr (STATS) {
          cs0 += a0; cs1 += a1; cs2 += a2; cs3 += a3;
          cq0 += a0 * a0; cq1 += a1 * a1; cq2 += a2 * a2; cq3 += a3 * a3;
        }
        if constexpr (OUT == 0) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, (f32x4_t){a0, a1, a2, a3}), rC, voc, 0, 0);
        } else {
          __builtin_amdgcn_raw_buffer_store_b64((u32x2_t){pack2<TC>(a0, a1), pack2<TC>(a2, a3)}, rC, voc, 0, 0);
        }
      }
      voc += stc;
    }
  }
  if constexpr (STATS) {
    // lanes l, l+16, l+32, l+48 hold the same 4 columns -> two wavefront shuffles; fixed order, reproducible
    cs0 += __shfl_xor(cs0, 16, 64); cs1 += __shfl_xor(cs1, 16, 64); cs2 += __shfl_xor(cs2, 16, 64); cs3 += __shfl_xor(cs3, 16, 64);
    cq0 += __shfl_xor(cq0, 16, 64); cq1 += __shfl_xor(cq1, 16, 64); cq2 += __shfl_xor(cq2, 16, 64); cq3 += __shfl_xor(cq3, 16, 64);
    cs0 += __shfl_xor(cs0, 32, 64); cs1 += __shfl_xor(cs1, 32, 64); cs2 += __shfl_xor(cs2, 32, 64); cs3 += __shfl_xor(cs3, 32, 64);
    cq0 += __shfl_xor(cq0, 32, 64); cq1 += __shfl_xor(cq1, 32, 64); cq2 += __shfl_xor(cq2, 32, 64); cq3 += __shfl_xor(cq3, 32, 64);
    if (stats_dst) {
      *(float4*)stats_dst = make_float4(cs0, cq0, cs1, cq1);
      *(float4*)(stats_dst + 4) = make_float4(cs2, cq2, cs3, cq3);
    }
  }
}



// Epilogue of the LDS-DMA kernels: the accumulators of a BM x BN tile (8 or 4 wavefronts, WM x WN) -> bias / time-embedding
// bias / residual / GEGLU / GroupNorm column statistics -> C, staged through this wave's 16 KiB slice of the (idle) LDS ring.
template <typename TC, int BM, int BN, int WM, int WN, bool MF16, int TI, int TJ>
__device__ __forceinline__ void dma_epilogue(const GemmParams& p, unsigned char* smem, f32x16 (&acc)[MF16 ? 1 : TI][MF16 ? 1 : TJ],
                                             f32x4_t (&acc16)[MF16 ? 8 : 1][MF16 ? 4 : 1], const int m0, const int n0, const int z0,
                                             const int z1, const int nsplit, const int ks, const int dbg) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int HW = p.H * p.W;

  // ---- epilogue ----------------------------------------------------------------------------------
  // The accumulators (row-per-register, column-per-lane) are staged through this wave's private
  // 16 KiB slice of the now idle LDS ring, 64 rows at a time, and read back row-contiguous, so
  // that bias / residual loads and the output stores are 16-byte vectors covering whole 256-byte
  // row segments (per-lane dword stores are store-issue bound: 64 instructions per wave, not 16).
  if ((dbg & 1) && (MF16 ? acc16[0][0][0] : acc[0][0][0]) != 123.456f) return;
  __builtin_amdgcn_s_barrier();                       // every wave is done reading the last stage
  float* stg = (float*)(smem + wave * 16384);         // [64 rows][64 cols] fp32
  const long coff = (long)z0 * p.sC_z0 + (long)z1 * p.sC_z1;
  const float* R = p.R ? (p.r_lowp ? (const float*)((const uint16_t*)p.R + (long)z0 * p.sR_z0 + (long)z1 * p.sR_z1)
                                   : p.R + (long)z0 * p.sR_z0 + (long)z1 * p.sR_z1) : nullptr;
  const bool need_b = p.bias_bn || p.r_up;
  const int rpb = p.rows_per_batch;
  const int b_first = need_b ? m0 / rpb : 0;          // a BM-row tile spans at most two samples when rpb >= BM
  const int b_edge = (b_first + 1) * rpb;
  const int cq = (lane & 15) * 4;                     // this lane's 4 columns inside a 64-column slab
  float* ws = nsplit > 1 ? (float*)p.ws + (long)ks * p.M * p.N : nullptr;

  // Lean path (every hot launch): operands addressed through buffer descriptors -- 32-bit per-lane
  // byte offsets bumped by a constant per 4-row step, rows past M dropped / zero-filled by the range
  // check -- and no per-row integer division.  The generic loop further down keeps the rare cases
  // (row bias, up-sampled residual, samples shorter than a tile, unaligned strides, >= 2 GiB operands).
  const int c_cols = p.geglu ? p.N / 2 : p.N;
  const long c_bytes = ws ? (long)p.M * p.N * 4 : ((long)(p.M - 1) * p.ldc + c_cols) * (p.c_f32 ? 4 : 2);
  const long r_rows = p.r_up ? (long)(p.M / HW) * (p.H >> 1) * (p.W >> 1) : (long)p.M;
  const long r_bytes = R ? ((r_rows - 1) * p.ldr + p.N) * (p.r_lowp ? 2 : 4) : 0;
  const bool lean = !(dbg & 512) && (p.N & 3) == 0 && c_bytes < (1L << 31) && r_bytes < (1L << 31) &&
                    (ws != nullptr || (!p.bias_m && (!need_b || rpb >= BM) && (p.geglu ? p.ldc % 2 == 0 : p.ldc % 4 == 0) &&
                                       (!R || p.ldr % 4 == 0) && (!p.bias_bn || p.ld_bn % 4 == 0)));
  const __amdgpu_buffer_rsrc_t rC =
      make_rsrc(ws ? (const void*)ws : (p.c_f32 ? (const void*)((float*)p.C + coff) : (const void*)((TC*)p.C + coff)), lean ? (int)c_bytes : 0);
  const __amdgpu_buffer_rsrc_t rR = make_rsrc(R ? (const void*)R : (const void*)p.C, lean ? (int)r_bytes : 0);
  const bool two_b = p.bias_bn && b_edge < m0 + BM && b_edge < p.M;   // the tile spans two samples

  // One 64 x 64 slab of the wave tile.  A generic lambda called with compile-time slab indices: the
  // accumulator arrays are then indexed by constants whatever the size of the body (a `#pragma unroll`
  // loop this large is silently left rolled, which sends the accumulators to scratch memory).
  auto slab = [&](auto HI, auto HJ) {
      constexpr int hi = decltype(HI)::value, hj = decltype(HJ)::value;
      if (hi + hj > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // previous slab fully read back
      if (!(dbg & 2048)) {
      if constexpr (MF16) {
        // transposed 16x16 accumulator (weights are the first MFMA operand): row = lane & 15, and register v of lane group
        // g = lane >> 4 in column tile j is channel 32 (j >> 1) + 8 g + 4 (j & 1) + v of the 64-column block (hperm)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            *(f32x4_t*)(stg + (i * 16 + (lane & 15)) * 64 + 32 * (j >> 1) + 8 * (lane >> 4) + 4 * (j & 1)) = acc16[4 * hi + i][4 * hj + j];
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v)
              stg[(i * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh) * 64 + j * 32 + lr] = acc[2 * hi + i][2 * hj + j][v];
      }
      }
      // same-wave LDS write -> read: the compiler orders them (lgkmcnt); no barrier needed
      const int row0 = m0 + wm * (BM / WM) + hi * 64;
      const int col = n0 + wn * (BN / WN) + hj * 64 + cq;
      if (lean) {
        const int rq = lane >> 4;
        const bool col_ok = col < p.N;                // N % 4 == 0: the lane's 4 columns are in or out together
        const float* sp = stg + rq * 64 + cq;
        const unsigned esz = (ws || p.c_f32) ? 4u : 2u;
        const unsigned ldc_e = ws ? (unsigned)p.N : (unsigned)p.ldc;
        const unsigned voc = (col_ok && !(dbg & 1024)) ? ((unsigned)(row0 + rq) * ldc_e + (unsigned)(p.geglu ? col >> 1 : col)) * esz : DMA_OOB;
        const unsigned stc = 4u * ldc_e * esz;
        const unsigned rsz = p.r_lowp ? 2u : 4u;
        const unsigned vor = col_ok ? ((unsigned)(row0 + rq) * (unsigned)p.ldr + (unsigned)col) * rsz : DMA_OOB;
        const unsigned str = 4u * rsz * (unsigned)p.ldr;
        const LeanRup rup = {p.r_up, p.W, HW, b_first, b_edge, (p.H >> 1) * (p.W >> 1), p.W >> 1, rsz * (unsigned)p.ldr, rsz * (unsigned)col};
        float4 bn0 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!ws && p.bias_n && col_ok) bn0 = *(const float4*)(p.bias_n + col);
        float4 bn1 = bn0;
        if (!ws && p.bias_bn && col_ok) {
          const float4 t = *(const float4*)(p.bias_bn + (long)b_first * p.ld_bn + col);
          bn0.x += t.x; bn0.y += t.y; bn0.z += t.z; bn0.w += t.w;
          if (two_b) {
            const float4 u = *(const float4*)(p.bias_bn + (long)(b_first + 1) * p.ld_bn + col);
            bn1.x += u.x; bn1.y += u.y; bn1.z += u.z; bn1.w += u.w;
          }
        }
        const int edge = two_b ? b_edge : 0x7fffffff;
        float* sd = (p.col_stats && lane < 16 && col_ok && row0 < p.M) ? p.col_stats + ((long)(row0 >> 6) * p.N + col) * 2 : nullptr;
#define T2P_LEAN(OUT, HR, ST)                                                                                             \
  do {                                                                                                                   \
    if (HR && p.r_lowp) lean_slab<TC, OUT, HR, ST, HR>(sp, rC, rR, voc, stc, vor, str, bn0, bn1, row0 + rq, edge, p.alpha, sd, rup); \
    else lean_slab<TC, OUT, HR, ST, false>(sp, rC, rR, voc, stc, vor, str, bn0, bn1, row0 + rq, edge, p.alpha, sd, rup); \
  } while (0)
        if (ws) T2P_LEAN(3, false, false);
        else if (p.geglu) T2P_LEAN(2, false, false);
        else if (p.c_f32) {
          if (R) { if (p.col_stats) T2P_LEAN(0, true, true); else T2P_LEAN(0, true, false); }
          else { if (p.col_stats) T2P_LEAN(0, false, true); else T2P_LEAN(0, false, false); }
        } else {
          if (R) { if (p.col_stats) T2P_LEAN(1, true, true); else T2P_LEAN(1, true, false); }
          else { if (p.col_stats) T2P_LEAN(1, false, true); else T2P_LEAN(1, false, false); }
        }
#undef T2P_LEAN
        return;
      }
      if (ws) {                                       // split-K: raw partial sums -> workspace [split][M][N]
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
          const int rl = it * 4 + (lane >> 4);
          const int row = row0 + rl;
          if (row >= p.M || col >= p.N) continue;
          const float4 a = *(const float4*)(stg + rl * 64 + cq);
          float* dst = ws + (long)row * p.N + col;
          if (col + 3 < p.N && (p.N & 3) == 0) *(float4*)dst = a;
          else {
            dst[0] = a.x;
            if (col + 1 < p.N) dst[1] = a.y;
            if (col + 2 < p.N) dst[2] = a.z;
            if (col + 3 < p.N) dst[3] = a.w;
          }
        }
        return;
      }
      const bool full4 = col + 3 < p.N;
      float4 bn = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p.bias_n) {
        if (full4) bn = *(const float4*)(p.bias_n + col);
        else {
          if (col < p.N) bn.x = p.bias_n[col];
          if (col + 1 < p.N) bn.y = p.bias_n[col + 1];
          if (col + 2 < p.N) bn.z = p.bias_n[col + 2];
        }
      }
      const bool vec_ok = full4 && (p.ldc % 4 == 0 || p.geglu) && (!R || p.ldr % 4 == 0) && (!p.bias_bn || p.ld_bn % 4 == 0);
      float cs0 = 0.f, cs1 = 0.f, cs2 = 0.f, cs3 = 0.f, cq0 = 0.f, cq1 = 0.f, cq2 = 0.f, cq3 = 0.f;   // column sums / sums of squares
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int rl = it * 4 + (lane >> 4);
        const int row = row0 + rl;
        if (row >= p.M || col >= p.N) continue;
        float4 a = *(const float4*)(stg + rl * 64 + cq);
        int bidx = 0;
        if (need_b) bidx = rpb >= BM ? b_first + (row >= b_edge ? 1 : 0) : row / rpb;
        long rrow = row;
        if (p.r_up) {
          const int rem = row - bidx * HW;
          const int y = rem / p.W, x = rem - y * p.W;
          rrow = ((long)bidx * (p.H >> 1) + (y >> 1)) * (p.W >> 1) + (x >> 1);
        }
        const float bm = p.bias_m ? p.bias_m[row] : 0.f;
        a.x += bm + bn.x; a.y += bm + bn.y; a.z += bm + bn.z; a.w += bm + bn.w;
        if (vec_ok) {
          if (p.bias_bn) {
            const float4 t = *(const float4*)(p.bias_bn + (long)bidx * p.ld_bn + col);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
          }
          if (R) {
            const float4 t = res_load4<TC>(R, rrow * p.ldr + col, p.r_lowp);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
          }
          if (p.geglu) {
            // columns are interleaved (value_j, gate_j): out[row][col / 2 + {0, 1}] = value * gelu_erf(gate)
            // (GEGLU.forward, reference model/attention.py:42-44), stored in the compute dtype
            const float g0 = 0.5f * a.y * (1.f + erff(a.y * 0.70710678118654752440f));
            const float g1 = 0.5f * a.w * (1.f + erff(a.w * 0.70710678118654752440f));
            TC* dst = (TC*)p.C + coff + (long)row * p.ldc + (col >> 1);
            union { TC e[2]; uint32_t u; } o;
            o.e[0] = from_f32<TC>(a.x * g0); o.e[1] = from_f32<TC>(a.z * g1);
            *(uint32_t*)dst = o.u;
            continue;
          }
          a.x *= p.alpha; a.y *= p.alpha; a.z *= p.alpha; a.w *= p.alpha;
          cs0 += a.x; cs1 += a.y; cs2 += a.z; cs3 += a.w;
          cq0 += a.x * a.x; cq1 += a.y * a.y; cq2 += a.z * a.z; cq3 += a.w * a.w;
          if (p.c_f32) {
            *(float4*)((float*)p.C + coff + (long)row * p.ldc + col) = a;
          } else {
            TC* dst = (TC*)p.C + coff + (long)row * p.ldc + col;
            union { TC e[4]; uint2 u; } o;
            o.e[0] = from_f32<TC>(a.x); o.e[1] = from_f32<TC>(a.y); o.e[2] = from_f32<TC>(a.z); o.e[3] = from_f32<TC>(a.w);
            *(uint2*)dst = o.u;
          }
        } else {
          float vals[4] = {a.x, a.y, a.z, a.w};
          for (int k = 0; k < 4; ++k) {
            if (col + k >= p.N) break;
            float val = vals[k];
            if (p.bias_bn) val += p.bias_bn[(long)bidx * p.ld_bn + col + k];
            if (R) val += res_load1<TC>(R, rrow * p.ldr + col + k, p.r_lowp);
            val *= p.alpha;
            if (p.c_f32) ((float*)p.C)[coff + (long)row * p.ldc + col + k] = val;
            else ((TC*)p.C)[coff + (long)row * p.ldc + col + k] = from_f32<TC>(val);
          }
        }
      }
      // GroupNorm statistics of the tensor just produced (consumed by gn_finalize_cols_kernel): per
      // 64-row chunk and column, sum and sum of squares of the final fp32 values.  Lanes l, l+16,
      // l+32, l+48 hold the same 4 columns -> two wavefront shuffles; fixed order, reproducible.
      if (p.col_stats) {
        cs0 += __shfl_xor(cs0, 16, 64); cs1 += __shfl_xor(cs1, 16, 64); cs2 += __shfl_xor(cs2, 16, 64); cs3 += __shfl_xor(cs3, 16, 64);
        cq0 += __shfl_xor(cq0, 16, 64); cq1 += __shfl_xor(cq1, 16, 64); cq2 += __shfl_xor(cq2, 16, 64); cq3 += __shfl_xor(cq3, 16, 64);
        cs0 += __shfl_xor(cs0, 32, 64); cs1 += __shfl_xor(cs1, 32, 64); cs2 += __shfl_xor(cs2, 32, 64); cs3 += __shfl_xor(cs3, 32, 64);
        cq0 += __shfl_xor(cq0, 32, 64); cq1 += __shfl_xor(cq1, 32, 64); cq2 += __shfl_xor(cq2, 32, 64); cq3 += __shfl_xor(cq3, 32, 64);
        if (lane < 16 && vec_ok) {
          float* dst = p.col_stats + ((long)(row0 >> 6) * p.N + col) * 2;
          *(float4*)dst = make_float4(cs0, cq0, cs1, cq1);
          *(float4*)(dst + 4) = make_float4(cs2, cq2, cs3, cq3);
        }
      }
  };
  slab(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
  if constexpr (TJ / 2 > 1) slab(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
  if constexpr (TI / 2 > 1) {
    slab(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
    if constexpr (TJ / 2 > 1) slab(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
  }
}

// ---- register epilogue of the 16x16x32 kernels ------------------------------------------------------------------------
// The 16x16x32 kernels feed the WEIGHT fragment as the MFMA's first operand, so that an accumulator tile comes out
// transposed: lane (m = lane & 15, g = lane >> 4) holds 4 consecutive OUTPUT CHANNELS (MFMA rows 4 g + v) of pixel row m.
// The weight rows of a wave's 64-column block are permuted while they are staged (hperm below): MFMA row 4 g + v of
// column tile j is channel 32 (j >> 1) + 8 g + 4 (j & 1) + v, so a lane owns channels [8 g, 8 g + 8) and
// [32 + 8 g, 32 + 8 g + 8) of its row: two 16-byte stores per 16-row tile in 16 bits, each instruction covering 16 rows
// x 64 contiguous bytes -- no LDS round trip (the staged epilogue writes 256 KiB of accumulators per tile through a
// 64 B/clk LDS store path and reads them back), half the store instructions, and the LDS ring stays free.
// (hperm: gemm_mfma.h)
// sum over the 16 lanes of a DPP row (lane & 15), fixed order: every lane ends with the total
__device__ __forceinline__ float row16_sum(float x) {
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, false));  // row_half_mirror
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, false));  // row_mirror
  return x;
}

#ifndef T2P_C_AUX
#define T2P_C_AUX 0          // cache policy of the register epilogue's 16-bit output stores (measurement variants: 2 nt, 16 sc1, 17 sc0 sc1)
#endif
// The GemmParams of a gemm_dma / gemm_dxs kernel as they sit in the kernel-argument segment (the struct is the FIRST argument of every
// kernel that carries the register epilogue), behind an empty asm so that the compiler treats the pointer as opaque
typedef __attribute__((address_space(4))) GemmParams KernArgs;
__device__ __forceinline__ const KernArgs* kernel_args() {
  const KernArgs* pk = (const KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(pk));
  return pk;
}
// PLAIN: the caller knows at compile time that the launch is the network's common case -- 16-bit output, no split-K workspace, no GEGLU,
// no per-row bias, no up-sampling phase: the per-tile uniform branches on those (a dozen per 16-row tile) and their scalar bookkeeping
// fold away.  Same arithmetic, same order: bit-identical to the general form.
template <typename TC, int BM, int BN, int WM, int WN, bool CFRAG = false, bool PLAIN = false, typename PT = GemmParams>
__device__ __forceinline__ void reg_epilogue(const PT& p, f32x4_t (&acc16)[8][4], const int m0, const int n0, const int z0,
                                             const int z1, const int nsplit, const int ks, const int dbg) {
  if ((dbg & 1) && acc16[0][0][0] != 123.456f) return;
  int tx = threadIdx.x;
  asm volatile("" : "+v"(tx));       // nothing lane-derived of the epilogue is computed before the K loop and kept across it (registers)
  const int lane = tx & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tx >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int HW = p.H * p.W;
  const long coff = (long)z0 * p.sC_z0 + (long)z1 * p.sC_z1;
  const float* R = p.R ? (p.r_lowp ? (const float*)((const uint16_t*)p.R + (long)z0 * p.sR_z0 + (long)z1 * p.sR_z1)
                                   : p.R + (long)z0 * p.sR_z0 + (long)z1 * p.sR_z1) : nullptr;
  static_assert(!(PLAIN && CFRAG), "the plain form stores row-major only");
  float* ws = (!PLAIN && nsplit > 1) ? (float*)p.ws + (long)ks * p.M * p.N : nullptr;
  const bool p_geglu = PLAIN ? false : p.geglu != 0, p_c_f32 = PLAIN ? false : p.c_f32 != 0;
  const float* const p_bias_m = PLAIN ? nullptr : p.bias_m;
  const int c_cols = p_geglu ? p.N / 2 : p.N;
  const long c_bytes = ws ? (long)p.M * p.N * 4 : ((long)(p.M - 1) * p.ldc + c_cols) * (p_c_f32 ? 4 : 2);
  const long r_rows = p.r_up ? (long)(p.M / HW) * (p.H >> 1) * (p.W >> 1) : (long)p.M;
  const long r_bytes = R ? ((r_rows - 1) * p.ldr + p.N) * (p.r_lowp ? 2 : 4) : 0;
  const __amdgpu_buffer_rsrc_t rC =
      make_rsrc(ws ? (const void*)ws : (p_c_f32 ? (const void*)((float*)p.C + coff) : (const void*)((TC*)p.C + coff)), (int)c_bytes);
  const __amdgpu_buffer_rsrc_t rR = make_rsrc(R ? (const void*)R : (const void*)p.C, (int)r_bytes);

  const int row_w = m0 + wm * (BM / WM);                 // first row of the wave tile (128 rows = 8 tiles of 16)
  // up_phase (MODE 3): rows are pixels of the half-resolution map; row (b, yl, xl) is stored at output pixel (b, 2 yl + py, 2 xl + px)
  const int upp = PLAIN ? 0 : (p.up_phase == 5 ? 1 + (int)blockIdx.y : p.up_phase);     // 5: all four phases in one launch, the phase on grid.y
  const int Mrows = upp ? p.M >> 2 : p.M;
  const int Wl = p.W >> 1, HWl = (p.H >> 1) * (p.W >> 1);
  const int col0 = n0 + wn * (BN / WN) + 8 * g4;         // this lane's channels: [col0, col0 + 8) and [col0 + 32, col0 + 40)
  const bool ok0 = col0 < p.N, ok1 = col0 + 32 < p.N;    // N % 8 == 0: a group of 8 channels is in or out as a whole
  // per-channel constants: bias_n + the time-embedding bias of the tile's first sample
  float bs[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) bs[k] = 0.f;
  const int rpb = p.rows_per_batch;
  const bool need_b = p.bias_bn || p.r_up;
  const int b_first = upp ? m0 / HWl : (need_b ? m0 / rpb : 0);
  if (!ws) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = col0 + 32 * h;
      if (c < p.N) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p.bias_n) t = *(const float4*)(p.bias_n + c + 4 * q);
          if (p.bias_bn) {
            const float4 a = *(const float4*)(p.bias_bn + (long)b_first * p.ld_bn + c + 4 * q);
            t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w;
          }
          const int k = 8 * h + 4 * q;
          bs[k] = t.x; bs[k + 1] = t.y; bs[k + 2] = t.z; bs[k + 3] = t.w;
        }
      }
    }
  }
  const unsigned esz = (ws || p_c_f32) ? 4u : 2u;
  const unsigned ldc_e = ws ? (unsigned)p.N : (unsigned)p.ldc;
  const unsigned rsz = p.r_lowp ? 2u : 4u;
  const bool nostore = (dbg & 1024) != 0;
  const bool alpha_not_one = p.alpha != 1.0f;
  float cs[16], cq[16];                                   // GroupNorm column sums of a 64-row chunk (4 row tiles)

  // rows of 16-row tile i: the output row of this lane and (r_up) the half-resolution residual row
  auto rows_of = [&](int i, int& row, unsigned& rrow, int& bsel) __attribute__((always_inline)) {
    row = row_w + 16 * i + l16;
    bsel = 0;
    rrow = (unsigned)row;
    if (upp) {                                            // wave-uniform; Wl % 16 == 0: a tile's 16 rows share (b, yl)
      const int rt = row_w + 16 * i;
      const int bidx = rt / HWl, rem = rt - bidx * HWl, yl = rem / Wl, xl = rem - yl * Wl;
      bsel = bidx - (m0 / HWl);
      row = rt < Mrows ? (bidx * p.H + 2 * yl + ((upp - 1) >> 1)) * p.W + 2 * (xl + l16) + ((upp - 1) & 1) : p.M;
      rrow = (unsigned)row;
    } else if (need_b) {
      const int rt = row_w + 16 * i;                      // wave-uniform: the 16 rows of a tile lie in one sample (rpb % 16 == 0)
      const int bidx = rt / rpb;
      bsel = bidx - b_first;                              // 0 inside the tile's first sample
      if (p.r_up) {
        const int rem = rt - bidx * HW, y = rem / p.W, x = rem - y * p.W;     // x % 16 == 0 (W % 16 == 0)
        rrow = (unsigned)((bidx * (p.H >> 1) + (y >> 1)) * (p.W >> 1) + ((x + l16) >> 1));
      }
    }
  };
  // residual of one tile -> registers (RM 1: 16-bit residual, two 16-byte loads; RM 2: fp32, four)
  auto load_res = [&](auto RMC, int i, u32x4_t* rr) __attribute__((always_inline)) {
    constexpr int RM = decltype(RMC)::value;
    int row, bsel; unsigned rrow;
    rows_of(i, row, rrow, bsel);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned off = ((h ? ok1 : ok0) && row < p.M) ? (rrow * (unsigned)p.ldr + (unsigned)(col0 + 32 * h)) * rsz : DMA_OOB;
      if constexpr (RM == 1) {
        rr[h] = __builtin_amdgcn_raw_buffer_load_b128(rR, off, 0, 0);
      } else {
        rr[2 * h] = __builtin_amdgcn_raw_buffer_load_b128(rR, off, 0, 0);
        rr[2 * h + 1] = __builtin_amdgcn_raw_buffer_load_b128(rR, off == DMA_OOB ? DMA_OOB : off + 16, 0, 0);
      }
    }
  };
  // one 16-row tile; IC is a compile-time index so that the accumulators stay in registers
  auto tile = [&](auto IC, auto RMC, const u32x4_t* rr) __attribute__((always_inline)) {
    constexpr int i = decltype(IC)::value;
    constexpr int RM = decltype(RMC)::value;
    int row, bsel; unsigned rrow;
    rows_of(i, row, rrow, bsel);
    float v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = acc16[i][j][e];       // v[k]: channel col0 + (k & 7) + 32 (k >> 3)
    if (!ws) {
      float bm = 0.f;
      if (p_bias_m) bm = row < p.M ? p_bias_m[row] : 0.f;
      if (p.bias_bn && bsel > 0) {                       // the tile runs into a following sample (small maps): per-tile reload
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int c = col0 + (k & 7) + 32 * (k >> 3);
          v[k] += bm + (c < p.N ? (p.bias_n ? p.bias_n[c] : 0.f) + p.bias_bn[(long)(b_first + bsel) * p.ld_bn + c] : 0.f);
        }
      } else if constexpr (PLAIN) {                      // (no per-row bias: bm is zero)
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] += bs[k];
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] += bm + bs[k];
      }
      if constexpr (RM == 1) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4_t a = unpack4<TC>((u32x2_res_t){rr[h][0], rr[h][1]}), b = unpack4<TC>((u32x2_res_t){rr[h][2], rr[h][3]});
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[8 * h + e] += a[e]; v[8 * h + 4 + e] += b[e]; }
        }
      } else if constexpr (RM == 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4_t a = __builtin_bit_cast(f32x4_t, rr[2 * h]), b = __builtin_bit_cast(f32x4_t, rr[2 * h + 1]);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[8 * h + e] += a[e]; v[8 * h + 4 + e] += b[e]; }
        }
      }
    }
    const bool rok = row < p.M && !nostore;
    if (!ws && p_geglu) {
      // interleaved (value, gate) columns: out[row][c / 2] = value * gelu_erf(gate)  (GEGLU.forward, model/attention.py:42-44)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned off = ((h ? ok1 : ok0) && rok) ? ((unsigned)row * ldc_e + (unsigned)((col0 + 32 * h) >> 1)) * 2u : DMA_OOB;
        const float* w = v + 8 * h;
        __builtin_amdgcn_raw_buffer_store_b64((u32x2_t){pack2<TC>(w[0] * gelu_erf_fast(w[1]), w[2] * gelu_erf_fast(w[3])),
                                                         pack2<TC>(w[4] * gelu_erf_fast(w[5]), w[6] * gelu_erf_fast(w[7]))}, rC, off, 0, 0);
      }
      return;
    }
    if (!ws) {
      if (!PLAIN || alpha_not_one) {                     // (x * 1 = x exactly: skipping the product changes nothing)
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] *= p.alpha;
      }
      if (p.col_stats) {
        if (row < p.M) {
#pragma unroll
          for (int k = 0; k < 16; ++k) { cs[k] += v[k]; cq[k] += v[k] * v[k]; }
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned off = ((h ? ok1 : ok0) && rok) ? ((unsigned)row * ldc_e + (unsigned)(col0 + 32 * h)) * esz : DMA_OOB;
      const float* w = v + 8 * h;
      if (esz == 4u) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, (f32x4_t){w[0], w[1], w[2], w[3]}), rC, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, (f32x4_t){w[4], w[5], w[6], w[7]}), rC, off == DMA_OOB ? DMA_OOB : off + 16, 0, 0);
      } else {
        const u32x4_t packed = {pack2<TC>(w[0], w[1]), pack2<TC>(w[2], w[3]), pack2<TC>(w[4], w[5]), pack2<TC>(w[6], w[7])};
        if constexpr (CFRAG) {
          // columns from frag_col0 on: fragment-major (GemmParams::c_frag).  The 16 rows of a tile lie in one sample (rpb % 16 == 0)
          const int c = col0 + 32 * h - p.frag_col0;              // wave-uniform sign: frag_col0 % 64 == 0
          if (c >= 0) {
            const int rt = row_w + 16 * i;
            const int bz = p.rows_per_batch > 1 ? rt / p.rows_per_batch : z0;
            const int rl = row - (p.rows_per_batch > 1 ? bz * p.rows_per_batch : 0);
            const long e = (long)bz * p.frag_bstride + ((long)(rl >> 5) * p.frag_ns + (c >> 5)) * 1024 + ((c >> 3) & 1) * 512 + ((c >> 4) & 1) * 256 +
                           (rl & 31) * 8;
            if ((h ? ok1 : ok0) && rok) *(u32x4_t*)((TC*)p.c_frag + e) = packed;
            continue;
          }
        }
        __builtin_amdgcn_raw_buffer_store_b128(packed, rC, off, 0, T2P_C_AUX);
      }
    }
  };
  // GroupNorm statistics of a 64-row chunk: column sums folded over the 16 lanes of a row group, written by lane m = 0
  auto flush_stats = [&](int chunk_row) __attribute__((always_inline)) {
    if (!p.col_stats || ws) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) { cs[k] = row16_sum(cs[k]); cq[k] = row16_sum(cq[k]); }
    if (l16 == 0 && chunk_row < Mrows) {
      long chunk = chunk_row >> 6;
      if (upp) {            // the consumer sums the HW / 64 chunks of a sample: a phase fills its quarter of each sample's range
        const int bidx = chunk_row / HWl;
        chunk = (long)bidx * ((p.H * p.W) >> 6) + (long)(upp - 1) * (HWl >> 6) + ((chunk_row - bidx * HWl) >> 6);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h ? ok1 : ok0) {
          float* dst = p.col_stats + (chunk * p.N + col0 + 32 * h) * 2;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            *(float4*)(dst + 4 * q) = make_float4(cs[8 * h + 2 * q], cq[8 * h + 2 * q], cs[8 * h + 2 * q + 1], cq[8 * h + 2 * q + 1]);
        }
      }
    }
  };
  // a half of the wave tile (4 row tiles = one statistics chunk); the residual rows are requested ahead of their use:
  // three tiles ahead in 16 bits (6 loads in flight), two tiles at a time in fp32 (8 loads)
  auto half = [&](auto HC, auto RMC) __attribute__((always_inline)) {
    constexpr int i0 = 4 * decltype(HC)::value;
    constexpr int RM = decltype(RMC)::value;
#pragma unroll
    for (int k = 0; k < 16; ++k) cs[k] = cq[k] = 0.f;
    if constexpr (RM == 1) {
      u32x4_t rr[3][2];                                  // three tiles requested ahead (registers: 229 + these must stay <= 256)
      load_res(RMC, i0, rr[0]); load_res(RMC, i0 + 1, rr[1]); load_res(RMC, i0 + 2, rr[2]);
      tile(std::integral_constant<int, i0>{}, RMC, rr[0]);
      load_res(RMC, i0 + 3, rr[0]);
      tile(std::integral_constant<int, i0 + 1>{}, RMC, rr[1]); tile(std::integral_constant<int, i0 + 2>{}, RMC, rr[2]);
      tile(std::integral_constant<int, i0 + 3>{}, RMC, rr[0]);
    } else if constexpr (RM == 2) {
      u32x4_t rr[2][4];
      load_res(RMC, i0, rr[0]); load_res(RMC, i0 + 1, rr[1]);
      tile(std::integral_constant<int, i0>{}, RMC, rr[0]); tile(std::integral_constant<int, i0 + 1>{}, RMC, rr[1]);
      load_res(RMC, i0 + 2, rr[0]); load_res(RMC, i0 + 3, rr[1]);
      tile(std::integral_constant<int, i0 + 2>{}, RMC, rr[0]); tile(std::integral_constant<int, i0 + 3>{}, RMC, rr[1]);
    } else {
      tile(std::integral_constant<int, i0>{}, RMC, nullptr); tile(std::integral_constant<int, i0 + 1>{}, RMC, nullptr);
      tile(std::integral_constant<int, i0 + 2>{}, RMC, nullptr); tile(std::integral_constant<int, i0 + 3>{}, RMC, nullptr);
    }
    flush_stats(row_w + 16 * i0);
  };
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
  if (!R || ws) { half(I0{}, I0{}); half(I1{}, I0{}); }
  else if (p.r_lowp) { half(I0{}, I1{}); half(I1{}, I1{}); }
  else { half(I0{}, I2{}); half(I1{}, I2{}); }
}

// MF16: use v_mfma_f32_16x16x32 (sustains a higher clock than 32x32x16 at equal cycles per FLOP in
// LDS-fed loops, MI355X_MICROARCH.md "DVFS give-back" item 7) -- 128 x 64 wave tiles only.
template <typename TC, int BM, int BN, int WM, int WN, int MODE, int NST, int NSTB, bool MF16, bool REGE, bool CFRAG>
__device__ __forceinline__ void gemm_dma_body(const GemmParams& p, const int tiles_m, const int tiles_n, const int dbg_arg) {
  // dbg: timing-only ablation mask.  Bits 128 / 256 change the DMA issue order only (results unchanged); every
  // other bit skips work and gives wrong results: those exist in -DT2P_ABLATION builds only (never shipped).
#ifdef T2P_ABLATION
  const int dbg = dbg_arg;
#else
  const int dbg = dbg_arg & (128 | 256 | 4096 | 8192);
#endif
  // NST stages for the A (activation) tile, NSTB for the B (weight) tile.  NSTB < NST gives the
  // activations -- which come from L2 / Infinity Cache -- a longer lead than the L2-hot weights
  // within the 160 KiB of LDS (256 x 256: 3 x 32 KiB + 2 x 32 KiB).
  constexpr int BK = 64;
  constexpr int NW = WM * WN;
  constexpr int TI = BM / WM / 32, TJ = BN / WN / 32;  // 32x32 MFMA tiles per wave
  static_assert(NW == 8 || NW == 4, "4 or 8 wavefronts");
  static_assert((TI == 2 || TI == 4) && (TJ == 2 || TJ == 4) && TI * TJ <= 8, "wave tile");
  static_assert(NW * 16384 <= NST * BM * 128 + NSTB * BN * 128, "epilogue staging must fit the ring");
  static_assert(NSTB == NST || NSTB == NST - 1, "B ring is as deep as the A ring or one stage shallower");
  static_assert(!MF16 || (TI == 4 && TJ == 2), "the 16x16x32 variant is written for 128 x 64 wave tiles");
  constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;  // DMA instructions per wave per K-tile (8 rows each)
  constexpr int ASTAGE = BM * 128, BSTAGE = BN * 128;
  constexpr int BRING = NST * ASTAGE;                            // byte offset of the B ring
  constexpr int TAPS = MODE == 0 ? 1 : (MODE == 3 ? 4 : 9);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;

  // XCD-aware tile order: blocks b and b + 8 share an XCD; give each XCD a contiguous tile range
  const int ntiles = tiles_m * tiles_n;
  int tile = blockIdx.x;
  {
    const int q = ntiles >> 3, r = ntiles & 7, xcd = tile & 7, idx = tile >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  // MODE 3: the four output phases of an up-sampling convolution are the y dimension of one grid (up_phase == 5): a phase
  // launch of a low-resolution level has 64 workgroups, the four together fill the chip
  const int upk = MODE == 3 ? (p.up_phase == 5 ? 1 + (int)blockIdx.y : p.up_phase) : 0;
  const int z0 = MODE == 3 ? 0 : blockIdx.y / p.nz1, z1 = MODE == 3 ? 0 : blockIdx.y % p.nz1;

  const int Ctot = p.C0 + p.C1;
  const int nch = (Ctot + BK - 1) / BK;
  // MODE 1 only: an extra K segment read at the centre tap from X0 | X1 (the 1x1 shortcut of a residual block folded into its
  // second convolution): nchx more 64-channel K-tiles after the nch * 9 main ones
  const int nchx = MODE == 1 ? (p.CX0 + p.CX1) / BK : 0;
  const int nk_all = nch * TAPS + nchx;
  // split-K: blockIdx.z owns K-tiles [kt_lo, kt_hi) and writes a raw fp32 partial tile
  const int nsplit = gridDim.z, ks = blockIdx.z;
  const int kt_lo = (int)((long)nk_all * ks / nsplit), kt_hi = (int)((long)nk_all * (ks + 1) / nsplit);
  const int nk = kt_hi - kt_lo;
  const int HW = p.H * p.W;
  const int Hs = MODE >= 2 ? (p.H >> 1) : p.H, Ws = MODE >= 2 ? (p.W >> 1) : p.W;
  // MODE 3: one output phase (py, px) of a 3x3 convolution on a 2x nearest-up-sampled map = a 2x2 convolution on the
  // half-resolution map (the taps that read the same source pixel are summed into one weight on the host): rows are the
  // M / 4 source pixels, tap (ty, tx) reads pixel (yl + ty - 1 + py, xl + tx - 1 + px), the epilogue scatters row
  // (b, yl, xl) to output pixel (b, 2 yl + py, 2 xl + px).  4 / 9 of the multiplications of the gather form (MODE 2).
  const int up_py = MODE == 3 ? ((upk - 1) >> 1) : 0, up_px = MODE == 3 ? ((upk - 1) & 1) : 0;
  const int Mq = MODE == 3 ? p.M >> 2 : p.M;            // rows of this launch
  const int HWq = MODE == 3 ? Hs * Ws : HW, Wq = MODE == 3 ? Ws : p.W, Hq = MODE == 3 ? Hs : p.H;

  // buffer descriptors: whole operand in range, everything else reads as zero.  Built from
  // readfirstlane'd scalars so that hipcc keeps them in SGPRs (no waterfall loop around the DMA).
  const long a_rows = MODE == 0 ? (long)p.M : (long)(p.M / HW) * Hs * Ws;
  const TC* A0p = (const TC*)p.A0 + (long)z0 * p.sA_z0 + (long)z1 * p.sA_z1;
  const TC* Bp = (const TC*)p.Bw + (long)z0 * p.sB_z0 + (long)z1 * p.sB_z1 +
                 ((MODE == 3 && p.up_phase == 5) ? (long)(upk - 1) * p.N * p.ldb : 0L);       // phase weights [4][N][ldb]
  const int a0_bytes = (int)(((a_rows - 1) * p.lda0 + p.C0) * 2);
  const int a1_bytes = p.A1 ? (int)(((a_rows - 1) * p.lda1 + p.C1) * 2) : 0;
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(Bp, (int)((((long)p.N - 1) * p.ldb + (long)TAPS * Ctot + nchx * BK) * 2));
  const unsigned lda0_2 = (unsigned)(p.lda0 * 2), lda1_2 = (unsigned)(p.lda1 * 2);
  const unsigned ldx0_2 = (unsigned)(p.ldx0 * 2), ldx1_2 = (unsigned)(p.ldx1 * 2);
  // (fields copied out: `c ? p.a : p.b` is an lvalue conditional -- an address select into the by-value argument struct, which
  // then lands in scratch memory)
  const void* const X0p = p.X0; const void* const X1p = p.X1; const void* const A1p = p.A1;
  const int pC0 = p.C0, pCX0 = p.CX0;
  const int x0_bytes = nchx ? (int)((((long)p.M - 1) * p.ldx0 + p.CX0) * 2) : 0;
  const int x1_bytes = (nchx && p.X1) ? (int)((((long)p.M - 1) * p.ldx1 + p.CX1) * 2) : 0;

  // per-lane DMA geometry: instruction j of this wave covers tile rows (wave * INSTR + j) * 8 + (lane >> 3).
  // K order is chunk-major (all 9 taps of one 64-channel slice back to back: the 3x3 window
  // re-reads stay in the XCD's L2).  For MODE 1 the source row of tap (dy, dx) is m + dy*W + dx
  // (NHWC rows are pixel-major), so per K-tile the lane adds one wave-uniform byte delta to a
  // precomputed offset; bit t of a_vm says whether tap t lands inside the map.
  const int prow = lane >> 3, ppos = lane & 7;
  // a lane keeps the row m of each of its instructions (24-bit: offset = m * row stride + chunk through one v_mad_u32_u24,
  // whatever the source), the swizzled chunk offset (it depends on the parity of j only) and the tap-validity bits
  static_assert(A_INSTR % 2 == 0, "the chunk swizzle of instruction j depends on j & 1 only when A_INSTR is even");
  unsigned a_m[A_INSTR], a_vm[A_INSTR], a_chk[2];
  int a_y[A_INSTR], a_x[A_INSTR], a_bb[A_INSTR];       // MODE 2 only
  a_chk[0] = (unsigned)((ppos ^ ((prow >> 1) & 7)) * 16);
  a_chk[1] = (unsigned)((ppos ^ ((4 + (prow >> 1)) & 7)) * 16);
#pragma unroll
  for (int j = 0; j < A_INSTR; ++j) {
    const int r = (wave * A_INSTR + j) * 8 + prow;
    const int m = m0 + r;
    unsigned vm = 0;
    int y = 0, x = 0, b = 0;
    if (MODE != 0) {
      b = m / HWq;
      const int rem = m - b * HWq;
      y = rem / Wq;
      x = rem - y * Wq;
    }
    if (m < Mq) {
      if (MODE == 0) {
        vm = 1;
      } else if (MODE == 3) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int sy = y + (t >> 1) - 1 + up_py, sx = x + (t & 1) - 1 + up_px;
          if (sy >= 0 && sy < Hq && sx >= 0 && sx < Wq) vm |= 1u << t;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int sy = y + t / 3 - 1, sx = x + t % 3 - 1;
          if (sy >= 0 && sy < p.H && sx >= 0 && sx < p.W) vm |= 1u << t;
        }
      }
    }
    a_vm[j] = vm;
    a_y[j] = y; a_x[j] = x; a_bb[j] = b * Hs * Ws;
    a_m[j] = (unsigned)m;                            // MODE 2 recomputes the row per tap
  }
  unsigned b_off[B_INSTR];
#pragma unroll
  for (int j = 0; j < B_INSTR; ++j) {
    const int r = (wave * B_INSTR + j) * 8 + prow;
    const int n = n0 + (MF16 ? (r & ~63) + hperm(r & 63) : r);     // 16x16x32: permuted channels (see reg_epilogue)
    b_off[j] = n < p.N ? (unsigned)((long)n * p.ldb * 2) + (unsigned)((ppos ^ ((r >> 1) & 7)) * 16) : DMA_OOB;
  }

  // Issue-stream state (wave-uniform, SGPRs).  The A and the B stream are each issued strictly in K order, every K-tile once,
  // so each stream carries the position of its NEXT K-tile along: (chunk, tap, ring stage) plus everything an issue needs in
  // ready-made form -- the source's buffer descriptor and row stride (they change with the 64-channel chunk), and the
  // wave-uniform byte offset of the tap, advanced by one row stride per tap.  The common case of an issue is then a handful of
  // scalar additions; the recomputation at a chunk boundary sits in a block that one issue in nine enters (the empty asm
  // statements keep the compiler from turning those blocks into select chains executed every time).  The scalar prelude of
  // an issue is what the two waves of a SIMD cannot hide from each other: ten more scalar instructions per issue measured
  // 3.7 % on the convolutions.
  int ia_chunk = kt_lo / TAPS, ia_tap = kt_lo - (kt_lo / TAPS) * TAPS;
  if (nchx && kt_lo >= nch * TAPS) { ia_chunk = nch + (kt_lo - nch * TAPS); ia_tap = 0; }     // a K-split that starts in the extra segment
  int ib_chunk = ia_chunk, ib_tap = ia_tap;
  unsigned ia_so = 0, ib_so = 0;                        // ring stage byte offsets
  int ia_dx = 0;                                        // MODE 1: column of the tap (-1, 0, 1): the row of taps ends after dx = 1
  __amdgpu_buffer_rsrc_t rA = make_rsrc(A0p, a0_bytes);
  unsigned a_ld2 = lda0_2, a_delta = 0, a_rowstep = 0;
  bool a_extra = false;
  // descriptor / stride / offsets of chunk ia_chunk, tap ia_tap
  auto a_set_chunk = [&]() __attribute__((always_inline)) {
    const bool extra = MODE == 1 && ia_chunk >= nch;   // K-tile of the shortcut segment (centre tap of X0 | X1)
    const int c0 = (extra ? ia_chunk - nch : ia_chunk) * BK;     // channel base of this K-tile
    int cfirst = pC0;
    if (extra) cfirst = pCX0;
    const bool second = c0 >= cfirst;                  // C0 % 64 == 0
    const int csrc = second ? c0 - cfirst : c0;
    // (plain assignments: a nested `c ? a : b` over named variables is an address select that keeps them in memory)
    unsigned ld2 = lda0_2;
    const void* abase = (const void*)A0p;
    int abytes = a0_bytes;
    if (extra) {
      if (second) { ld2 = ldx1_2; abase = X1p; abytes = x1_bytes; } else { ld2 = ldx0_2; abase = X0p; abytes = x0_bytes; }
    } else if (second) {
      ld2 = lda1_2; abase = A1p; abytes = a1_bytes;
    }
    rA = make_rsrc(abase, abytes);
    a_ld2 = ld2;
    a_extra = extra;
    int dy = 0, dx = 0;
    if (MODE == 1) {
      if (extra) { ia_tap = 4; ia_dx = 1; }            // tap 4 = the centre; dx = 1: the next advance leaves the "row of taps"
      else { dy = ia_tap / 3 - 1; dx = ia_tap - (ia_tap / 3) * 3 - 1; ia_dx = dx; }
      a_rowstep = (unsigned)(Wq - 3) * ld2;            // from (dy, dx = 2) to (dy + 1, -1)
    } else if (MODE == 3) {
      dy = (ia_tap >> 1) - 1 + up_py; dx = (ia_tap & 1) - 1 + up_px;
      a_rowstep = (unsigned)(Wq - 2) * ld2;            // from (ty, tx = 2) to (ty + 1, 0)
    }
    a_delta = (unsigned)((dy * Wq + dx) * (int)ld2 + csrc * 2);
  };
  a_set_chunk();
  const int a_switch = p.A1 ? pC0 / BK : 0x7fffffff;    // MODE 0: the chunk at which the second source starts
  const unsigned Ctot2 = (unsigned)(Ctot * 2);
  unsigned b_kb = (MODE == 1 && ib_chunk >= nch) ? (unsigned)(((long)TAPS * Ctot + (ib_chunk - nch) * BK) * 2)
                                                 : (unsigned)(((long)ib_tap * Ctot + ib_chunk * BK) * 2);
  if (MODE == 1 && ib_chunk >= nch) ib_tap = TAPS - 1;
  auto issue = [&](int /* kl: the streams keep their own position */, int part) __attribute__((always_inline)) {   // part 0: A rows, 1: B rows, 2: both
    if (part != 1) {
      unsigned char* sta = smem + ia_so;
      if constexpr (MODE == 2) {
        const int dy = ia_tap / 3 - 1, dx = ia_tap - (ia_tap / 3) * 3 - 1;
#pragma unroll
        for (int j = 0; j < A_INSTR; ++j) {
          const int row = a_bb[j] + ((a_y[j] + dy) >> 1) * Ws + ((a_x[j] + dx) >> 1);
          const unsigned voff = (unsigned)row * a_ld2 + a_delta + a_chk[j & 1];     // a_delta: the channel offset only
          const unsigned m = (dbg & 64) ? 0u : (unsigned)__builtin_amdgcn_sbfe((int)a_vm[j], (unsigned)ia_tap, 1u);
          unsigned char* dst = sta + (wave * A_INSTR + j) * 1024;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, T2P_LDS_PTR(dst), 16, (voff & m) | (DMA_OOB & ~m), 0, 0, 0);
        }
      } else {
        const unsigned vb0 = a_chk[0] + a_delta, vb1 = a_chk[1] + a_delta;
#pragma unroll
        for (int j = 0; j < A_INSTR; ++j) {
          const unsigned voff = __umul24(a_m[j], a_ld2) + ((j & 1) ? vb1 : vb0);     // rows and strides are below 2^24 (dma_eligible)
          // tap validity: bit ia_tap of a_vm[j] spread over the word (v_bfe_i32), then offset-or-out-of-range in one bit-select
          const unsigned m = (dbg & 64) ? 0u : (unsigned)__builtin_amdgcn_sbfe((int)a_vm[j], (unsigned)ia_tap, 1u);
          unsigned char* dst = sta + (wave * A_INSTR + j) * 1024;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, T2P_LDS_PTR(dst), 16, (voff & m) | (DMA_OOB & ~m), 0, 0, 0);
        }
      }
      if constexpr (NST == 2) ia_so ^= (unsigned)ASTAGE;
      else ia_so = ia_so + ASTAGE == NST * ASTAGE ? 0u : ia_so + ASTAGE;
      // advance to the next K-tile of the stream
      if constexpr (MODE == 0) {
        ++ia_chunk; a_delta += BK * 2;
        if (ia_chunk == a_switch) { asm volatile(""); a_set_chunk(); }
      } else if constexpr (MODE == 1) {
        ++ia_tap; ++ia_dx; a_delta += a_ld2;
        if (ia_dx > 1) {
          asm volatile("");
          ia_dx = -1; a_delta += a_rowstep;
          if (ia_tap == TAPS || a_extra) { asm volatile(""); ia_tap = 0; ++ia_chunk; a_set_chunk(); }
        }
      } else if constexpr (MODE == 3) {
        ++ia_tap; a_delta += a_ld2;
        if (!(ia_tap & 1)) {
          asm volatile("");
          a_delta += a_rowstep;
          if (ia_tap == TAPS) { asm volatile(""); ia_tap = 0; ++ia_chunk; a_set_chunk(); }
        }
      } else {
        ++ia_tap;
        if (ia_tap == TAPS) { asm volatile(""); ia_tap = 0; ++ia_chunk; a_set_chunk(); }
      }
    }
    if (part != 0) {
      unsigned char* stb = smem + BRING + ib_so;
#pragma unroll
      for (int j = 0; j < B_INSTR; ++j) {
        const unsigned voff = (dbg & 64) ? DMA_OOB : b_off[j] + b_kb;   // rows beyond N carry DMA_OOB: adding b_kb (< 2 GiB) keeps them out of range
        unsigned char* dst = stb + (wave * B_INSTR + j) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, T2P_LDS_PTR(dst), 16, voff, 0, 0, 0);
      }
      if constexpr (NSTB == 2) ib_so ^= (unsigned)BSTAGE;
      else ib_so = ib_so + BSTAGE == NSTB * BSTAGE ? 0u : ib_so + BSTAGE;
      if constexpr (TAPS == 1) {
        ++ib_chunk; b_kb += BK * 2;
      } else {
        ++ib_tap; b_kb += Ctot2;
        if (ib_tap == TAPS) {
          asm volatile("");
          ++ib_chunk;
          if (MODE == 1 && ib_chunk >= nch) { b_kb = (unsigned)(((long)TAPS * Ctot + (ib_chunk - nch) * BK) * 2); ib_tap = TAPS - 1; }
          else { ib_tap = 0; b_kb += (unsigned)(BK * 2) - (unsigned)TAPS * Ctot2; }
        }
      }
    }
  };

  f32x16 acc[MF16 ? 1 : TI][MF16 ? 1 : TJ];
  f32x4_t acc16[MF16 ? 8 : 1][MF16 ? 4 : 1];      // 16x16 tiles: row tile i (16 rows), column tile j (16 columns)
  if constexpr (MF16) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
  }

  // fragment read offsets: row (wave row base + i*32 + lr), chunk (2 s + lh) ^ ((row >> 1) & 7)
  // (the i-th 32-row tile of a wave is i * 4096 bytes further and has the same swizzle term,
  // so it is reached through the ds_read immediate offset)
  unsigned a_fo[4], b_fo[4];
  {
    const int ra = wm * (BM / WM) + lr, rb = wn * (BN / WN) + lr;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      a_fo[s] = (unsigned)(ra * 128 + (((2 * s + lh) ^ ((ra >> 1) & 7)) << 4));
      b_fo[s] = (unsigned)(BRING + rb * 128 + (((2 * s + lh) ^ ((rb >> 1) & 7)) << 4));
    }
  }

  // 16x16x32: lane (r = lane & 15, g = lane >> 4) reads 16 bytes of row (tile base + r) at logical
  // chunk 4 ks + g of the 128-byte K-slice; tile i is i * 16 rows = i * 2048 bytes further (same
  // swizzle term), reached through the immediate offset
  unsigned a16[2], b16[2];
  {
    const int r = lane & 15, g = lane >> 4;
    const int ra = wm * (BM / WM) + r, rb = wn * (BN / WN) + r;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      a16[ks] = (unsigned)(ra * 128 + (((4 * ks + g) ^ ((ra >> 1) & 7)) << 4));
      b16[ks] = (unsigned)(BRING + rb * 128 + (((4 * ks + g) ^ ((rb >> 1) & 7)) << 4));
    }
  }

  const unsigned lds_base = (unsigned)(unsigned long long)T2P_LDS_PTR(smem);
  // Issue order per iteration kt: B(kt + AB) first, then A(kt + AA).  vmcnt counts in order, so at
  // the top of iteration kt everything up to and including A(kt) and B(kt) has landed when at most
  // the loads issued after them are outstanding.
  constexpr int AA = NST - 1, AB = NSTB - 1;            // lead (K-tiles) of the A and B streams
  static_assert(AA <= 3 && (NSTB == NST || AA == 2), "ring depths: 2, 3 or 4 symmetric stages, or 3 + 2");
  issue(0, 2);
  if (AA > 1 && nk > 1) issue(1, AB > 1 ? 2 : 0);
  if (AA > 2 && nk > 2) issue(2, 2);
  unsigned ra_so = 0, rb_so = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // outstanding after A(kt), B(kt) in issue order: symmetric ring: the min(AA - 1, nk - 1 - kt) younger tiles (the tail of
    // the loop has fewer); asymmetric (AB == AA - 1): only A(kt + 1 .. kt + AA - 1)
    const int young = nk - 1 - kt;
    if (AA > 2 && young >= 2) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (A_INSTR + B_INSTR)) : "memory");
    } else if (AA > 1 && young >= 1) {
      if (NSTB == NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_INSTR + B_INSTR) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AA - 1) * A_INSTR) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (!(dbg & 8)) __builtin_amdgcn_s_barrier();
    const bool more_a = kt + AA < nk && !(dbg & 2), more_b = kt + AB < nk && !(dbg & 2);
    if (dbg & 4) { if (more_b) issue(kt + AB, 1); if (more_a) issue(kt + AA, 0); continue; }
    // Fragment reads go through inline asm: hipcc would otherwise put `s_waitcnt vmcnt(0)` in
    // front of every ds_read that may alias an in-flight LDS-DMA write and drain the ring.  The
    // reads of k-step s+1 are in flight while the MFMAs of step s run (lgkmcnt counts LDS ops in
    // order: <= TI + TJ outstanding means step s has landed).
    const unsigned sa_off = lds_base + ra_so, sb_off = lds_base + rb_so;      // ring stages of K-tile kt
    if constexpr (NST == 2) ra_so ^= (unsigned)ASTAGE;
    else ra_so = ra_so + ASTAGE == NST * ASTAGE ? 0u : ra_so + ASTAGE;
    if constexpr (NSTB == 2) rb_so ^= (unsigned)BSTAGE;
    else rb_so = rb_so + BSTAGE == NSTB * BSTAGE ? 0u : rb_so + BSTAGE;
    if constexpr (MF16) {
      // fragments: B of k-step 0 / 1 (4 column tiles each), A low / high half (4 row tiles each)
      u32x4_t B0[4], B1[4], AL[4], AH[4];
#define T2P_RD4(F, ADDR, I0)                                                                        \
  lds_read_b128_2k<I0>(F[0], ADDR); lds_read_b128_2k<I0 + 1>(F[1], ADDR);                            \
  lds_read_b128_2k<I0 + 2>(F[2], ADDR); lds_read_b128_2k<I0 + 3>(F[3], ADDR);
#define T2P_W8(N, X, Y)                                                                             \
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(Y[0]), "+v"(Y[1]), \
               "+v"(Y[2]), "+v"(Y[3]) : "n"(N));
#define T2P_M16(A, B, I0)                                                                           \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j)       \
      Mma16<TC>::run(B[j], A[i], acc16[I0 + i][j]);
      const unsigned aa0 = sa_off + a16[0], aa1 = sa_off + a16[1], bb0 = sb_off + b16[0], bb1 = sb_off + b16[1];
      // Waves w and w+4 share a SIMD.  The second half of the workgroup issues all of its DMA before
      // its matrix work, the first half in between: the two waves of a SIMD then run different
      // phases (one in the matrix pipe while the other issues DMA / waits on LDS), not in lockstep.
      const bool early = g_stagger_dbg(dbg) && wave >= (WM * WN) / 2;
      const bool late = g_stagger_dbg(dbg) && !(dbg & 256) && !early;
      if (early) {
        if (more_b) issue(kt + AB, 1);
        if (more_a) issue(kt + AA, 0);
      }
      T2P_RD4(B0, bb0, 0)
      T2P_RD4(AL, aa0, 0)
      T2P_RD4(AH, aa0, 4)
      T2P_W8(4, B0, AL)
      T2P_M16(AL, B0, 0)
      if (!early && !late && more_b) issue(kt + AB, 1);
      T2P_RD4(AL, aa1, 0)
      T2P_W8(4, B0, AH)
      T2P_M16(AH, B0, 4)
      if (!early && !late && more_a) issue(kt + AA, 0);
      if (late && more_b) issue(kt + AB, 1);
      T2P_RD4(B1, bb1, 0)
      T2P_RD4(AH, aa1, 4)
      T2P_W8(4, B1, AL)
      T2P_M16(AL, B1, 0)
      if (late && more_a) issue(kt + AA, 0);
      T2P_W8(0, B1, AH)
      T2P_M16(AH, B1, 4)
#undef T2P_RD4
#undef T2P_W8
#undef T2P_M16
      continue;
    }
    u32x4_t fa0[TI], fb0[TJ], fa1[TI], fb1[TJ];
#define T2P_RD(S, FA, FB)                                                                          \
  {                                                                                                \
    const unsigned aa = sa_off + a_fo[S];                                                          \
    const unsigned ba = sb_off + b_fo[S];                                                          \
    lds_read_b128<0>(FA[0], aa);                                                                   \
    lds_read_b128<0>(FB[0], ba);                                                                   \
    lds_read_b128<1>(FA[1], aa);                                                                   \
    lds_read_b128<1>(FB[1], ba);                                                                   \
    if constexpr (TI == 4) { lds_read_b128<2>(FA[2], aa); lds_read_b128<3>(FA[3], aa); }           \
    if constexpr (TJ == 4) { lds_read_b128<2>(FB[2], ba); lds_read_b128<3>(FB[3], ba); }           \
  }
#define T2P_WAIT(N, FA, FB)                                                                                           \
  if constexpr (TI == 2 && TJ == 2)                                                                                   \
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(FA[0]), "+v"(FA[1]), "+v"(FB[0]), "+v"(FB[1]) : "n"(N));              \
  else if constexpr (TI == 4)                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(%6)"                                                                              \
                 : "+v"(FA[0]), "+v"(FA[1]), "+v"(FA[2]), "+v"(FA[3]), "+v"(FB[0]), "+v"(FB[1]) : "n"(N));            \
  else                                                                                                                \
    asm volatile("s_waitcnt lgkmcnt(%6)"                                                                              \
                 : "+v"(FA[0]), "+v"(FA[1]), "+v"(FB[0]), "+v"(FB[1]), "+v"(FB[2]), "+v"(FB[3]) : "n"(N));
#define T2P_MMA(FA, FB)                                                                            \
  _Pragma("unroll") for (int i = 0; i < TI; ++i) _Pragma("unroll") for (int j = 0; j < TJ; ++j)    \
      Mma<TC>::run(__builtin_bit_cast(uint4, FA[i]), __builtin_bit_cast(uint4, FB[j]), acc[i][j]);
    // The fragment reads start right after the barrier; the DMA of the next K-tile (address
    // VALU + buffer_load...lds) is issued between MFMA groups so that it overlaps the matrix
    // pipe instead of holding every wave of the workgroup in a VALU-only phase.
    constexpr int NRD = TI + TJ;
    const bool early = WM * WN == 8 && g_stagger_dbg(dbg) && wave >= 4;   // see the 16x16x32 loop above
    if (early) {
      if (more_b) issue(kt + AB, 1);
      if (more_a) issue(kt + AA, 0);
    }
    T2P_RD(0, fa0, fb0)
    T2P_RD(1, fa1, fb1)
    T2P_WAIT(NRD, fa0, fb0)
    T2P_MMA(fa0, fb0)
    if (!early && more_b) issue(kt + AB, 1);
    T2P_RD(2, fa0, fb0)
    T2P_WAIT(NRD, fa1, fb1)
    T2P_MMA(fa1, fb1)
    if (!early && more_a) issue(kt + AA, 0);
    T2P_RD(3, fa1, fb1)
    T2P_WAIT(NRD, fa0, fb0)
    T2P_MMA(fa0, fb0)
    T2P_WAIT(0, fa1, fb1)
    T2P_MMA(fa1, fb1)
#undef T2P_RD
#undef T2P_WAIT
#undef T2P_MMA
  }

  // REGE (16x16x32 kernels; chosen by the launcher with reg_epilogue_ok): epilogue straight from the registers
  if constexpr (MF16 && REGE) {
    // The epilogue reads its parameters from the kernel-argument segment through a pointer the compiler cannot see through (KernArgs):
    // it then loads each field where it is used (s_load from the constant cache) instead of keeping three dozen of them in scalar
    // registers across the K loop -- which it did by spilling them to VGPR lanes (25 v_writelane, 3700 v_readlane per kernel).
    // plain products (MODE 0: the attention / MLP projections, 8 K-tiles at C = 512, where the epilogue is a quarter of a tile) take the
    // specialised form when the launch is its case; the convolution modes keep one epilogue each (code size, registers)
    const KernArgs* pk = kernel_args();
    if constexpr (MODE == 0 && !CFRAG) {
      if (nsplit == 1 && !(dbg & 8192) && !pk->geglu && !pk->c_f32 && !pk->bias_m && !pk->up_phase)
        reg_epilogue<TC, BM, BN, WM, WN, false, true, KernArgs>(*pk, acc16, m0, n0, z0, z1, 1, 0, dbg);
      else reg_epilogue<TC, BM, BN, WM, WN, CFRAG, false, KernArgs>(*pk, acc16, m0, n0, z0, z1, nsplit, ks, dbg);
    } else {
      reg_epilogue<TC, BM, BN, WM, WN, CFRAG, false, KernArgs>(*pk, acc16, m0, n0, z0, z1, nsplit, ks, dbg);
    }
  }
  else dma_epilogue<TC, BM, BN, WM, WN, MF16, TI, TJ>(p, smem, acc, acc16, m0, n0, z0, z1, nsplit, ks, dbg);
}
template <typename TC, int BM, int BN, int WM, int WN, int MODE, int NST, int NSTB = NST, bool MF16 = false, bool REGE = false>
__global__ __launch_bounds__(WM * WN * 64) void gemm_dma_kernel(const GemmParams p, const int tiles_m, const int tiles_n, const int dbg_arg) {
  gemm_dma_body<TC, BM, BN, WM, WN, MODE, NST, NSTB, MF16, REGE, false>(p, tiles_m, tiles_n, dbg_arg);
}
// the same kernel writing part of its output fragment-major (GemmParams::c_frag; register epilogue only)
template <typename TC, int BM, int BN, int WM, int WN, int MODE, int NST, int NSTB>
__global__ __launch_bounds__(WM * WN * 64) void gemm_dma_cfrag_kernel(const GemmParams p, const int tiles_m, const int tiles_n, const int dbg_arg) {
  gemm_dma_body<TC, BM, BN, WM, WN, MODE, NST, NSTB, true, true, true>(p, tiles_m, tiles_n, dbg_arg);
}

// =================================================================================================
// v4 (round 4): 3x3 convolution at full resolution with the three HORIZONTAL taps of a window row served from one LDS stage.
//
// In the implicit GEMM above every input element lands in LDS nine times, once per tap: 96 KiB of activations per 64-channel chunk
// and 256 x 256 tile, 4.8 GB of L2 -> LDS traffic per launch on cfg2's dominant layer; that stream costs the loop a quarter of its
// matrix rate (1.57 -> 1.16 PFLOP/s, section 8 of DESIGN.md).  NHWC rows are pixel-major, so the rows a tile needs for tap
// (dy, dx) are the rows of tap (dy, 0) shifted by dx: ONE stage [rows m + dy W of the tile] serves dx = -1, 0, +1 when the
// fragment reads address row r + dx.  The two things that made the round-2 LDS-halo kernel lose are absent here:
//   * no halo and no padding: a tile is whole image rows (BM % W == 0), so the rows r - 1 of the tile's first pixel and r + 1 of its
//     last one are image-row edges, where the tap is zero anyway -- the stage is exactly the BM rows the kernel above stages;
//   * the image-row edges inside a tile (x = 0 under dx = -1, x = W - 1 under dx = +1) cost four v_cndmask per affected 16-pixel
//     tile and 32-deep step: with W a multiple of 64 only tiles 0 / 4 (left) and 3 / 7 (right) of a wave's 128 rows can be edges,
//     a wave-uniform test each; no per-lane tap bookkeeping.
// K order, weights layout, MFMA order and the register epilogue are those of gemm_dma_kernel<.., 1, 2, 2, true, true>: the results
// are bit-identical.  Activation DMA drops to one third (one stage per (chunk, dy) instead of per tap) and has two K-tiles to land
// instead of one; the weight stream is unchanged.  The 1x1 shortcut segment (X0 | X1) rides as single-tap groups at the end.
#ifdef T2P_ABLATION
// in-kernel timeline of the dx-shared kernel (measurement builds only): per tile, s_memtime of wave 0 at entry, before the K loop, after
// the first K-tile's data landed, after the K loop, after the epilogue issued its stores and after they drained
constexpr int DXS_STAMP_TILES = 4096, DXS_STAMPS = 8;
static __device__ unsigned long long g_dxs_stamps[DXS_STAMP_TILES * DXS_STAMPS];      // one per translation unit; the f16 one is read
#define T2P_STAMP(K) do { if (blockIdx.x < DXS_STAMP_TILES && threadIdx.x == 0) g_dxs_stamps[blockIdx.x * DXS_STAMPS + (K)] = __builtin_amdgcn_s_memtime(); } while (0)
#define T2P_STAMP_RT(K) do { if (blockIdx.x < DXS_STAMP_TILES && threadIdx.x == 0) g_dxs_stamps[blockIdx.x * DXS_STAMPS + (K)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define T2P_STAMP(K) do { } while (0)
#define T2P_STAMP_RT(K) do { } while (0)
#endif
template <typename TC, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void gemm_dxs_body(const GemmParams& p, const int tiles_m, const int tiles_n, const int dbg_arg) {
  const int dbg = dbg_arg & (128 | 256);
  constexpr int BK = 64, NW = WM * WN;
  static_assert(NW == 8 && BM / WM == 128 && BN / WN == 64, "128 x 64 wave tiles, 8 wavefronts");
  constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;
  // LDS: the weight ring FIRST, then the activation ring: row -1 of an activation stage (read by lane r = 0 of a wave's first tile under
  // dx = -1, always an image-row edge, always zeroed) is then ordinary LDS memory, not an address below the allocation
  constexpr int ASTAGE = BM * 128, BSTAGE = BN * 128, ARING = 2 * BSTAGE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  T2P_STAMP(0);
  T2P_STAMP_RT(6);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int ntiles = tiles_m * tiles_n;
  int tile = blockIdx.x;
  {
    const int q = ntiles >> 3, r = ntiles & 7, xcd = tile & 7, idx = tile >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int Ctot = p.C0 + p.C1, nch = Ctot / BK, nchx = (p.CX0 + p.CX1) / BK;
  const int ngroups = nch * 3 + nchx;                 // A stages: (chunk, dy) x 3 K-tiles each, then the shortcut chunks x 1 K-tile
  const int HW = p.H * p.W, W = p.W;

  const TC* A0p = (const TC*)p.A0;
  const TC* Bp = (const TC*)p.Bw;
  const long a_rows = p.M;
  const int a0_bytes = (int)(((a_rows - 1) * p.lda0 + p.C0) * 2);
  const int a1_bytes = p.A1 ? (int)(((a_rows - 1) * p.lda1 + p.C1) * 2) : 0;
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(Bp, (int)((((long)p.N - 1) * p.ldb + 9L * Ctot + nchx * BK) * 2));
  const unsigned lda0_2 = (unsigned)(p.lda0 * 2), lda1_2 = (unsigned)(p.lda1 * 2);
  const unsigned ldx0_2 = (unsigned)(p.ldx0 * 2), ldx1_2 = (unsigned)(p.ldx1 * 2);
  const void* const X0p = p.X0; const void* const X1p = p.X1; const void* const A1p = p.A1;
  const int pC0 = p.C0, pCX0 = p.CX0;
  const int x0_bytes = nchx ? (int)((((long)p.M - 1) * p.ldx0 + p.CX0) * 2) : 0;
  const int x1_bytes = (nchx && p.X1) ? (int)((((long)p.M - 1) * p.ldx1 + p.CX1) * 2) : 0;

  // DMA geometry.  The row of instruction j is a_m0 + 8 j (per lane).  The 8 rows of an instruction lie in one image row (W % 8 == 0) and
  // the tile in one sample (HW % BM == 0), so the validity of its three window rows is WAVE-UNIFORM: a_vmp, a scalar, packs it for all
  // instructions (bit 3 j + dy + 1: 0 <= y + dy < H; every row is < M since M % BM == 0) -- two integer divisions per tile, on the
  // scalar unit, instead of two per instruction and lane
  const int prow = lane >> 3, ppos = lane & 7;
  // activation swizzle: 16-byte chunk c of stage row r sits at chunk c ^ (r & 6).  ds_read_b128 is served in the lane groups
  // {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32): rows {0-3, 12-15} at chunk c together with rows {4-11} at chunk c ^ 1.  The
  // usual (r >> 1) & 7 term is conflict-free for that only while lane parity = row parity; under the +-1 row shift of the dx taps it
  // is 2-way on a quarter of the slots (SQ_LDS_BANK_CONFLICT 19.9 M per launch at 256x256).  r & 6 is conflict-free at all three
  // shifts (and has period 8: one source offset for every instruction).
  const unsigned a_chk = (unsigned)((ppos ^ (prow & 6)) * 16);
  const unsigned a_m0 = (unsigned)(m0 + wave * A_INSTR * 8 + prow);
  unsigned a_vmp;
  static_assert(A_INSTR * 3 <= 32, "validity bits of a wave's A instructions fit one register");
  {
    const int lgW = 31 - __builtin_clz(W);              // W is a power of two (dxs_eligible)
    const int b = m0 / HW, y0 = (m0 - b * HW) >> lgW, Hm1 = p.H - 1;
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < A_INSTR; ++j) {
      const int y = y0 + (((wave * A_INSTR + j) * 8) >> lgW);
      v |= ((y > 0 ? 1u : 0u) | 2u | (y < Hm1 ? 4u : 0u)) << (3 * j);
    }
    a_vmp = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
  }
  unsigned b_off[B_INSTR];
#pragma unroll
  for (int j = 0; j < B_INSTR; ++j) {
    const int r = (wave * B_INSTR + j) * 8 + prow;
    const int n = n0 + (r & ~63) + hperm(r & 63);
    b_off[j] = n < p.N ? (unsigned)((long)n * p.ldb * 2) + (unsigned)((ppos ^ ((r >> 1) & 7)) * 16) : DMA_OOB;
  }

  // ---- A stream: one stage per group --------------------------------------------------------------------------------------
  int ga = 0;                                           // next group to issue
  unsigned ia_so = 0;
  auto issue_a = [&]() __attribute__((always_inline)) {
    const bool extra = ga >= nch * 3;
    const int chunk = extra ? ga - nch * 3 : ga / 3;
    const int dyi = extra ? 1 : ga - chunk * 3;         // window row 0 .. 2 (the shortcut segment reads the output pixel itself)
    const int c0 = chunk * BK;
    int cfirst = pC0;
    if (extra) cfirst = pCX0;
    const bool second = c0 >= cfirst;
    const int csrc = second ? c0 - cfirst : c0;
    unsigned ld2 = lda0_2;
    const void* abase = (const void*)A0p;
    int abytes = a0_bytes;
    if (extra) {
      if (second) { ld2 = ldx1_2; abase = X1p; abytes = x1_bytes; } else { ld2 = ldx0_2; abase = X0p; abytes = x0_bytes; }
    } else if (second) {
      ld2 = lda1_2; abase = A1p; abytes = a1_bytes;
    }
    const __amdgpu_buffer_rsrc_t rA = make_rsrc(abase, abytes);
    const unsigned delta = (unsigned)((dyi - 1) * W * (int)ld2 + csrc * 2);
    const unsigned base = __umul24(a_m0, ld2) + delta;
    const unsigned vb0 = a_chk + base;
    const unsigned step = 8u * ld2;                     // 8 rows further per instruction
    unsigned char* sta = smem + ARING + ia_so;
#pragma unroll
    for (int j = 0; j < A_INSTR; ++j) {
      const unsigned voff = vb0 + (unsigned)j * step;
      const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)a_vmp, (unsigned)(3 * j + dyi), 1u);
      unsigned char* dst = sta + (wave * A_INSTR + j) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, T2P_LDS_PTR(dst), 16, (voff & m) | (DMA_OOB & ~m), 0, 0, 0);
    }
    ia_so ^= (unsigned)ASTAGE;
    ++ga;
  };
  // ---- B stream: one stage per K-tile, K order (chunk, tap), then the shortcut columns ---------------------------------------
  int ib_chunk = 0, ib_tap = 0;
  unsigned ib_so = 0, b_kb = 0;
  const unsigned Ctot2 = (unsigned)(Ctot * 2);
  auto issue_b = [&]() __attribute__((always_inline)) {
    unsigned char* stb = smem + ib_so;
#pragma unroll
    for (int j = 0; j < B_INSTR; ++j) {
      unsigned char* dst = stb + (wave * B_INSTR + j) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, T2P_LDS_PTR(dst), 16, b_off[j] + b_kb, 0, 0, 0);
    }
    ib_so ^= (unsigned)BSTAGE;
    ++ib_tap; b_kb += Ctot2;
    if (ib_tap == 9) {
      asm volatile("");
      ++ib_chunk;
      if (ib_chunk >= nch) { b_kb = (unsigned)((9L * Ctot + (ib_chunk - nch) * BK) * 2); ib_tap = 8; }
      else { ib_tap = 0; b_kb += (unsigned)(BK * 2) - 9u * Ctot2; }
    }
  };

  f32x4_t acc16[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets: lane (r = lane & 15, g = lane >> 4) reads 16 bytes of row (wave rows + r + dx) at logical chunk 4 ks + g;
  // 16-row tile i is i * 2048 bytes further with the same swizzle term (immediate offset).  Rows -1 / BM of a stage are read only by
  // lanes the edge masks zero (they lie in the neighbouring ring stage / past the allocation, where LDS reads return zero).
  // (the second 32-deep step reads chunk 4 + g: the same offset with bit 6 flipped, (4 | g) ^ x = (g ^ x) ^ 4 -- one XOR per K-tile
  // instead of a second register per offset: four registers fewer through the K loop)
  unsigned a16[3], b16;
  {
    const int r = lane & 15, g = lane >> 4;
    const int rb = wn * (BN / WN) + r;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int ra = wm * (BM / WM) + r + d - 1;         // (-1 for the first lane of the first wave row under dx = -1)
      a16[d] = (unsigned)(ARING + ra * 128 + ((g ^ (ra & 6)) << 4));
    }
    b16 = (unsigned)(rb * 128 + ((g ^ ((rb >> 1) & 7)) << 4));
  }
  // image-row edges inside this wave's 128 rows (W % 64 == 0: only these four tiles can hold one)
  const int rowb = m0 + wm * (BM / WM);
  const bool eL0 = rowb % W == 0, eL4 = (rowb + 64) % W == 0, eR3 = eL4, eR7 = (rowb + 128) % W == 0;
  const bool is_r0 = (lane & 15) == 0, is_r15 = (lane & 15) == 15;
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  const unsigned lds_base = (unsigned)(unsigned long long)T2P_LDS_PTR(smem);
  const bool early = g_stagger_dbg(dbg) && wave >= NW / 2;
  const bool late = g_stagger_dbg(dbg) && !(dbg & 256) && !early;
  unsigned ra_so = 0, rb_so = 0;
  const int nk = nch * 9 + nchx;
  int kt = 0;                                           // K-tile being multiplied (B stream position kt + 1 is the next issue)
  bool a_requested = false;                             // the first K-tile of the running group requested the next group's stage

  // one K-tile: DX = 0 / 1 / 2 is the horizontal tap dx = DX - 1; `first`: first K-tile of its group (the next group's stage is
  // requested here, behind the weight tile, and has until the group's last K-tile to land: WAIT_A says whether it may still be in flight)
#define T2P_RD4(F, ADDR, I0)                                                                        \
  lds_read_b128_2k<I0>(F[0], ADDR); lds_read_b128_2k<I0 + 1>(F[1], ADDR);                            \
  lds_read_b128_2k<I0 + 2>(F[2], ADDR); lds_read_b128_2k<I0 + 3>(F[3], ADDR);
#define T2P_W8(N, X, Y)                                                                             \
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(Y[0]), "+v"(Y[1]), \
               "+v"(Y[2]), "+v"(Y[3]) : "n"(N));
#define T2P_M16(A, B, I0)                                                                           \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j)       \
      Mma16<TC>::run(B[j], A[i], acc16[I0 + i][j]);
  auto ktile = [&](auto DXC, auto FIRSTC, auto AFLYC) __attribute__((always_inline)) {
    constexpr int DX = decltype(DXC)::value;
    constexpr bool FIRST = decltype(FIRSTC)::value;     // issues the next group's A stage
    constexpr bool AFLY = decltype(AFLYC)::value;       // the A stage requested one K-tile ago may still be in flight at the top
    // (the weight tile of this K-tile was requested BEFORE the activation stage that may still be in flight: loads land in order, so
    // "at most the stage's A_INSTR loads outstanding" means the weight tile is there -- but only if that stage was requested at all)
    if (AFLY && a_requested) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_INSTR) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more_b = kt + 1 < nk, more_a = FIRST && ga < ngroups;
    if constexpr (FIRST) a_requested = more_a;
    const unsigned sa_off = lds_base + ra_so, sb_off = lds_base + rb_so;
    rb_so ^= (unsigned)BSTAGE;
    u32x4_t B0[4], B1[4], AL[4], AH[4];
    const unsigned aa0 = sa_off + a16[DX], aa1 = sa_off + (a16[DX] ^ 64u), bb0 = sb_off + b16, bb1 = sb_off + (b16 ^ 64u);
    if (early) {
      if (more_b) issue_b();
      if (more_a) issue_a();
    }
    T2P_RD4(B0, bb0, 0)
    T2P_RD4(AL, aa0, 0)
    T2P_RD4(AH, aa0, 4)
    T2P_W8(4, B0, AL)
    if constexpr (DX == 0) { if (eL0 && is_r0) AL[0] = zero4; }
    if constexpr (DX == 2) { if (eR3 && is_r15) AL[3] = zero4; }
    T2P_M16(AL, B0, 0)
    if (!early && !late && more_b) issue_b();
    T2P_RD4(AL, aa1, 0)
    T2P_W8(4, B0, AH)
    if constexpr (DX == 0) { if (eL4 && is_r0) AH[0] = zero4; }
    if constexpr (DX == 2) { if (eR7 && is_r15) AH[3] = zero4; }
    T2P_M16(AH, B0, 4)
    if (!early && !late && more_a) issue_a();
    if (late && more_b) issue_b();
    T2P_RD4(B1, bb1, 0)
    T2P_RD4(AH, aa1, 4)
    T2P_W8(4, B1, AL)
    if constexpr (DX == 0) { if (eL0 && is_r0) AL[0] = zero4; }
    if constexpr (DX == 2) { if (eR3 && is_r15) AL[3] = zero4; }
    T2P_M16(AL, B1, 0)
    if (late && more_a) issue_a();
    T2P_W8(0, B1, AH)
    if constexpr (DX == 0) { if (eL4 && is_r0) AH[0] = zero4; }
    if constexpr (DX == 2) { if (eR7 && is_r15) AH[3] = zero4; }
    T2P_M16(AH, B1, 4)
    ++kt;
  };
#undef T2P_RD4
#undef T2P_W8
#undef T2P_M16
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
  using Tt = std::true_type; using Ff = std::false_type;

  T2P_STAMP(1);
  issue_b();                                            // weight tile of K-tile 0
  issue_a();                                            // stage of group 0
  for (int g = 0; g < nch * 3; ++g) {
    ktile(I0{}, Tt{}, Ff{});                            // dx = -1: requests group g + 1
#ifdef T2P_ABLATION
    if (g == 0) T2P_STAMP(2);
#endif
    ktile(I1{}, Ff{}, Tt{});                            // dx =  0: only the weight tile has to be there
    ktile(I2{}, Ff{}, Ff{});                            // dx = +1
    ra_so ^= (unsigned)ASTAGE;
  }
  for (int e = 0; e < nchx; ++e) {                      // shortcut segment: one K-tile per stage, read at the output pixel
    ktile(I1{}, Tt{}, Ff{});
    ra_so ^= (unsigned)ASTAGE;
  }
  T2P_STAMP(3);
#ifdef T2P_ABLATION
  const int edbg = dbg_arg & 1024;                     // 1024: the stores go nowhere (timeline experiments)
#else
  const int edbg = 0;
#endif
  {
    const KernArgs* pk = kernel_args();                 // (see gemm_dma_body: the epilogue's parameters are loaded where they are used)
    if (!(dbg_arg & 8192) && !pk->c_f32 && !pk->bias_m) reg_epilogue<TC, BM, BN, WM, WN, false, true, KernArgs>(*pk, acc16, m0, n0, 0, 0, 1, 0, edbg);
    else reg_epilogue<TC, BM, BN, WM, WN, false, false, KernArgs>(*pk, acc16, m0, n0, 0, 0, 1, 0, edbg);
  }
#ifdef T2P_ABLATION
  T2P_STAMP(4);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  T2P_STAMP(5);
  T2P_STAMP_RT(7);
#endif
}
template <typename TC, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_dxs_kernel(const GemmParams p, const int tiles_m, const int tiles_n, const int dbg_arg) {
  gemm_dxs_body<TC, BM, BN, WM, WN>(p, tiles_m, tiles_n, dbg_arg);
}


template <typename TC, int MODE, int BM, int BN, int WM, int WN, int NST, int NSTB = NST, bool MF16 = false, bool REGE = false, bool CF = false>
static int launch_dma_geom(const GemmParams& p, hipStream_t stream) {
  constexpr int smem = NST * BM * 128 + NSTB * BN * 128;
  constexpr int threads = WM * WN * 64;
  if constexpr (MF16 && !REGE && MODE != 3) {          // the register epilogue wherever it covers the launch
    if (reg_epilogue_ok(p, dma_plan(p).nsplit, g_plan.dbg)) return launch_dma_geom<TC, MODE, BM, BN, WM, WN, NST, NSTB, true, true>(p, stream);
  }
  void (*kern)(const GemmParams, const int, const int, const int);
  if constexpr (CF) kern = gemm_dma_cfrag_kernel<TC, BM, BN, WM, WN, MODE, NST, NSTB>;     // part of the output fragment-major (GemmParams::c_frag)
  else kern = gemm_dma_kernel<TC, BM, BN, WM, WN, MODE, NST, NSTB, MF16, REGE>;
  T2P_TRY(ensure_dynamic_lds((const void*)kern, smem));
  const int Mq = MODE == 3 ? p.M / 4 : p.M;               // MODE 3: one output phase per launch
  const int tiles_m = (Mq + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int nsplit = MODE == 3 ? 1 : dma_plan(p).nsplit;
  dim3 grid(tiles_m * tiles_n, MODE == 3 ? (p.up_phase == 5 ? 4 : 1) : p.nz0 * p.nz1, nsplit);
  ProfScope prof;
  if (prof.on()) {
    ProfRec& rec = prof.rec;
    prof_shape(rec, p);
    rec.flops = MODE == 3 ? 2.0 * Mq * p.N * 4.0 * (p.C0 + p.C1) * (p.up_phase == 5 ? 4 : 1)     // the multiplications this launch executes
                          : 2.0 * p.M * p.N * ((double)p.taps * (p.C0 + p.C1) + p.CX0 + p.CX1) * p.nz0 * p.nz1;
    rec.kind = p.taps == 9 ? 0 : 1;
    static const std::string kname = std::string(CF ? "gemm_dma_cfrag_kernel<" : "gemm_dma_kernel<") + (dtype_of<TC>::value == DT_F16 ? "f16_t" : "bf16_t") + ", " +
                                     std::to_string(BM) + ", " + std::to_string(BN) + ", " + std::to_string(WM) + ", " + std::to_string(WN) +
                                     ", " + std::to_string(MODE) + ", " + std::to_string(NST) + ", " + std::to_string(NSTB) + ", " +
                                     (MF16 ? "true" : "false") + ", " + (REGE ? "true" : "false") + ">";
    rec.name = kname.c_str();
    {
      const double Ct = p.C0 + p.C1, z = (double)p.nz0 * p.nz1;
      const double a_rows = p.a_up ? p.M / 4.0 : p.M;                    // up-sampling convs gather from the half-resolution map
      const double Cx = p.CX0 + p.CX1;                                   // shortcut segment: its input rows and weights once
      rec.bytes = z * (a_rows * Ct * 2 + (double)p.N * p.taps * Ct * 2 + (double)p.M * Cx * 2 + (double)p.N * Cx * 2 +
                       (double)p.M * (p.geglu ? p.N / 2 : p.N) * (p.c_f32 ? 4 : 2) +
                       (p.R ? (double)p.M * p.N * (p.r_lowp ? 2 : 4) / (p.r_up ? 4 : 1) : 0.0) + (p.bias_bn ? (double)(p.M / p.rows_per_batch) * p.N * 4 : 0.0));
    }
  }
  T2P_TRY(prof.open(stream));
  hipLaunchKernelGGL(kern, grid, dim3(threads), smem, stream, p, tiles_m, tiles_n, g_plan.dbg);
  T2P_TRY(prof.close());                                         // the main kernel only: comparable with rocprofv3's per-kernel average
  if (nsplit > 1) T2P_TRY(launch_splitk_reduce(p, nsplit, stream));
  prof.commit();
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// the dx-shared-stage kernel applies: a 3x3 convolution at full resolution on the 16x16x32 geometries whose tiles are whole image rows
static bool dxs_eligible(const GemmParams& p, const DmaPlan& plan) {
  if (!g_plan.dxs || p.taps != 9 || p.a_up || plan.nsplit != 1 || (plan.geom != 1 && plan.geom != 3) || g_plan.dma_ring != 2) return false;
  if (p.nz0 * p.nz1 != 1 || p.c_frag || p.geglu) return false;
  const int BM = plan.geom == 1 ? 256 : 512, HW = p.H * p.W;
  if (p.W % 64 != 0 || (p.W & (p.W - 1)) != 0 || BM % p.W != 0 || HW % BM != 0 || p.M % HW != 0) return false;
  if ((p.CX0 + p.CX1) % 64 != 0) return false;
  return reg_epilogue_ok(p, 1, 0);            // the kernel carries the register epilogue only
}

template <typename TC, int BM, int BN, int WM, int WN>
static int launch_dxs(const GemmParams& p, hipStream_t stream) {
  constexpr int smem = 2 * BM * 128 + 2 * BN * 128;
  auto kern = gemm_dxs_kernel<TC, BM, BN, WM, WN>;
  T2P_TRY(ensure_dynamic_lds((const void*)kern, smem));
  const int tiles_m = p.M / BM, tiles_n = (p.N + BN - 1) / BN;
  ProfScope prof;
  if (prof.on()) {
    ProfRec& rec = prof.rec;
    prof_shape(rec, p);
    rec.flops = 2.0 * p.M * p.N * (9.0 * (p.C0 + p.C1) + p.CX0 + p.CX1);
    rec.kind = 0;
    static const std::string kname = std::string("gemm_dxs_kernel<") + (dtype_of<TC>::value == DT_F16 ? "f16_t" : "bf16_t") + ", " +
                                     std::to_string(BM) + ", " + std::to_string(BN) + ", " + std::to_string(WM) + ", " + std::to_string(WN) + ">";
    rec.name = kname.c_str();
    const double Ct = p.C0 + p.C1, Cx = p.CX0 + p.CX1;
    rec.bytes = (double)p.M * Ct * 2 + (double)p.N * 9 * Ct * 2 + (double)p.M * Cx * 2 + (double)p.N * Cx * 2 + (double)p.M * p.N * (p.c_f32 ? 4 : 2) +
                (p.R ? (double)p.M * p.N * (p.r_lowp ? 2 : 4) : 0.0) + (p.bias_bn ? (double)(p.M / p.rows_per_batch) * p.N * 4 : 0.0);
  }
  T2P_TRY(prof.open(stream));
  hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(WM * WN * 64), smem, stream, p, tiles_m, tiles_n, g_plan.dbg);
  T2P_TRY(prof.close());
  prof.commit();
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

// a 3x3 convolution on a 2x up-sampled map as four 2x2 convolutions on the source map (kernel MODE 3): the caller supplied
// the phase weights (GemmParams::Bw4), the 16x16x32 geometries with the register epilogue run it
static bool up4_eligible(const GemmParams& p, const DmaPlan& plan) {
  if (!g_plan.up4 || !p.Bw4 || p.taps != 9 || !p.a_up || plan.nsplit != 1 || (plan.geom != 1 && plan.geom != 3) || g_plan.dma_ring != 2) return false;
  if (p.nz0 * p.nz1 != 1 || p.R || p.bias_m || p.geglu || p.A1) return false;
  const int Ws = p.W / 2, HWs = (p.H / 2) * (p.W / 2);
  if (p.H % 2 || p.W % 2 || Ws % 16 != 0 || HWs % 64 != 0 || p.M % (p.H * p.W) != 0) return false;
  if (p.bias_bn && p.rows_per_batch != p.H * p.W) return false;
  if ((long)p.N * p.ldb4 * 2 * 4 >= (1L << 31) - 64) return false;
  return reg_epilogue_ok(p, 1, g_plan.dbg);
}

template <typename TC, int MODE>
int launch_dma_mode(const GemmParams& p, hipStream_t stream) {
  const DmaPlan plan = dma_plan(p);
  if constexpr (MODE == 0) {
    if (p.c_frag) {
      T2P_REQUIRE(gemm_writes_frag_major(p), "this product does not take the fragment-major output (ask gemm_writes_frag_major)");
      return launch_dma_geom<TC, 0, 256, 256, 2, 4, 2, 2, true, true, true>(p, stream);
    }
  }
  if constexpr (MODE == 2) {
    if (up4_eligible(p, plan)) {
      GemmParams q = p;
      q.ldb = p.ldb4;
      q.Bw = p.Bw4;
      q.up_phase = 5;                  // all four phases in one launch (grid.y = phase)
      if (plan.geom == 1) return launch_dma_geom<TC, 3, 256, 256, 2, 4, 2, 2, true, true>(q, stream);
      return launch_dma_geom<TC, 3, 512, 128, 4, 2, 2, 2, true, true>(q, stream);
    }
  }
  if constexpr (MODE == 1) {
    if (dxs_eligible(p, plan)) {
      if (plan.geom == 1) return launch_dxs<TC, 256, 256, 2, 4>(p, stream);
      return launch_dxs<TC, 512, 128, 4, 2>(p, stream);
    }
  }
  switch (plan.geom) {
    case 1:
      if (g_plan.dma_ring == 2) return launch_dma_geom<TC, MODE, 256, 256, 2, 4, 2, 2, true>(p, stream);   // 16x16x32 MFMA
      return launch_dma_geom<TC, MODE, 256, 256, 2, 4, 2>(p, stream);      // ring 1: the 32x32x16 MFMA shape on the same tile
    case 2: return launch_dma_geom<TC, MODE, 128, 128, 2, 2, 2>(p, stream);
    case 4: return launch_dma_geom<TC, MODE, 128, 128, 2, 2, 4>(p, stream);
    case 3:
      if (g_plan.dma_ring == 2) return launch_dma_geom<TC, MODE, 512, 128, 4, 2, 2, 2, true>(p, stream);
      return launch_dma_geom<TC, MODE, 512, 128, 4, 2, 2>(p, stream);
    default: return launch_dma_geom<TC, MODE, 256, 128, 4, 2, 3>(p, stream);
  }
}

// ---- explicit instantiations ------------------------------------------------------------------------
// build.py compiles this file once per -DT2P_DMA_INST=k, so that the six launch_dma_mode<dtype, MODE> build in parallel; without the
// macro one unit holds all six.
#ifndef T2P_DMA_INST
#define T2P_DMA_INST -1
#endif
#if T2P_DMA_INST == -1 || T2P_DMA_INST == 0
template int launch_dma_mode<f16_t, 0>(const GemmParams&, hipStream_t);
#endif
#if T2P_DMA_INST == -1 || T2P_DMA_INST == 1
template int launch_dma_mode<f16_t, 1>(const GemmParams&, hipStream_t);
#ifdef T2P_ABLATION
int dxs_stamps_read(unsigned long long* out, int n) {
  if (n > DXS_STAMP_TILES * DXS_STAMPS) n = DXS_STAMP_TILES * DXS_STAMPS;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dxs_stamps), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? n : -1;
}
#endif
#endif
#if T2P_DMA_INST == -1 || T2P_DMA_INST == 2
template int launch_dma_mode<f16_t, 2>(const GemmParams&, hipStream_t);
#endif
#if T2P_DMA_INST == -1 || T2P_DMA_INST == 3
template int launch_dma_mode<bf16_t, 0>(const GemmParams&, hipStream_t);
#endif
#if T2P_DMA_INST == -1 || T2P_DMA_INST == 4
template int launch_dma_mode<bf16_t, 1>(const GemmParams&, hipStream_t);
#endif
#if T2P_DMA_INST == -1 || T2P_DMA_INST == 5
template int launch_dma_mode<bf16_t, 2>(const GemmParams&, hipStream_t);
#endif

}  // namespace t2p
