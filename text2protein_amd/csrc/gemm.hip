// MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (see GemmParams in t2p_common.h).
//
// The GEMM units (shared device helpers and the declarations between them: gemm_device.h):
//   gemm.hip         this file: the register-staged gemm_kernel, the planner (dma_eligible, dma_plan, the gemm_fuses_* / gemm_can_* /
//                    gemm_rowres_planned predicates) and launch_gemm
//   gemm_dma.hip     the LDS-DMA kernels (gemm_dma_kernel, gemm_dxs_kernel), their epilogues and launch_dma_mode<dtype, MODE>;
//                    compiled once per instantiation (build.py)
//   gemm_splitk.hip  the second pass of the split-K plans
//   thin_conv.hip    the thin-output head convolution
//   launch_prof.h    the scope every launcher times its launch with (t2p_profile_*)
//
// Replaces, on the sampling path of the reference: nn.Conv2d 3x3 (layers.py:89-95), 1x1
// convolutions (layers.py:82-87, attention.py:233-248), NIN (layers.py:128-137), nn.Linear
// (attention.py:161-168, 40, 60) and the four einsum contractions of the attention blocks
// (layers.py:166-171, attention.py:181,191).
//
// Structure: one workgroup = 4 wavefronts (64 lanes each) computes a BM x BN tile; wave (wm, wn)
// owns a (BM/2) x (BN/2) sub-tile made of 32x32 MFMA tiles.  Operand tiles are staged
// global -> registers -> LDS (16-byte vectors, 144-byte padded rows so that ds_read_b128
// fragment reads and ds_write_b128 staging writes are bank-conflict free), double-buffered so
// the global loads of K-tile t+1 are in flight while the MFMAs of tile t run.
//   * fp32 compute : v_mfma_f32_32x32x2_f32  (exact f32, 64 FLOP/clk/SIMD)
//   * bf16 / fp16  : v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulate
// LDS rows hold BK = 128 bytes of K (32 fp32 / 64 16-bit elements); a lane's fragment for
// k-group s is the 16 bytes at [row][32 s + 16 (lane >> 5)], for both element widths.
#include <algorithm>

#include "gemm_device.h"
#include "launch_prof.h"
#include "t2p_kernels.h"

namespace t2p {

template <typename TC, bool AF32, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmParams p) {
  constexpr int VEC = VecInfo<TC>::VEC;
  constexpr int BK = 8 * VEC;
  constexpr int AR = BM / 32, BR = BN / 32;  // staging rows per thread
  constexpr int TM = BM / 64, TN = BN / 64;  // 32x32 MFMA tiles per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* As = smem;                          // [2][BM][ROWB]
  unsigned char* Bs = smem + 2 * BM * ROWB;          // [2][BN][ROWB]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int z0 = blockIdx.z / p.nz1, z1 = blockIdx.z % p.nz1;

  const int Ctot = p.C0 + p.C1;
  const int nch = (Ctot + BK - 1) / BK;
  const int nk = nch * p.taps;
  const bool spatial = (p.taps == 9) || p.a_up;
  const int HW = p.H * p.W;
  const int Hs = p.a_up ? (p.H >> 1) : p.H, Ws = p.a_up ? (p.W >> 1) : p.W;

  const long aoff = (long)z0 * p.sA_z0 + (long)z1 * p.sA_z1;
  const char* A0 = (const char*)p.A0 + aoff * (AF32 ? 4 : (long)sizeof(TC));
  const char* A1 = (const char*)p.A1;
  const TC* Bw = (const TC*)p.Bw + (long)z0 * p.sB_z0 + (long)z1 * p.sB_z1;

  // staging assignment: vector column cv (16 bytes of K), rows srow + 32 i
  const int cv = tid & 7, srow = tid >> 3;
  int a_b[AR], a_y[AR], a_x[AR];
  bool a_ok[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    int m = m0 + srow + 32 * i;
    a_ok[i] = m < p.M;
    if (spatial) {
      int b = m / HW, rem = m - b * HW;
      a_b[i] = b; a_y[i] = rem / p.W; a_x[i] = rem - a_y[i] * p.W;
    } else {
      a_b[i] = m; a_y[i] = 0; a_x[i] = 0;
    }
  }

  uint4 ra[AR], rb[BR];

  auto gload = [&](int kt) {
    const int tap = kt / nch;
    const int c = (kt - tap * nch) * BK + cv * VEC;
    const bool cok = c < Ctot;
    const int nvalid = Ctot - c;   // < VEC only for ragged K (taps == 1)
    int dy = 0, dx = 0;
    if (p.taps == 9) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
    const bool second = c >= p.C0;
    const void* src = second ? (const void*)A1 : (const void*)A0;
    const long ld = second ? p.lda1 : p.lda0;
    const int cc = second ? c - p.C0 : c;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      bool ok = a_ok[i] && cok;
      long row = a_b[i];
      if (spatial) {
        int sy = a_y[i] + dy, sx = a_x[i] + dx;
        ok = ok && sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
        if (p.a_up) { sy >>= 1; sx >>= 1; }
        row = ((long)a_b[i] * Hs + sy) * Ws + sx;
      }
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ok) {
        v = load_vec<TC, AF32>(src, row * ld + cc);
        if (nvalid < VEC) v = mask_tail<TC>(v, nvalid);
      }
      ra[i] = v;
    }
    const long kb = (long)tap * Ctot + c;
#pragma unroll
    for (int j = 0; j < BR; ++j) {
      int n = n0 + srow + 32 * j;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (n < p.N && cok) {
        v = *(const uint4*)(Bw + (long)n * p.ldb + kb);
        if (nvalid < VEC) v = mask_tail<TC>(v, nvalid);
      }
      rb[j] = v;
    }
  };
  auto sstore = [&](int buf) {
    unsigned char* a = As + buf * BM * ROWB;
    unsigned char* b = Bs + buf * BN * ROWB;
#pragma unroll
    for (int i = 0; i < AR; ++i) *(uint4*)(a + (srow + 32 * i) * ROWB + cv * 16) = ra[i];
#pragma unroll
    for (int j = 0; j < BR; ++j) *(uint4*)(b + (srow + 32 * j) * ROWB + cv * 16) = rb[j];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const unsigned char* a = As + buf * BM * ROWB + (wm * (BM / 2) + lr) * ROWB + lh * 16;
    const unsigned char* b = Bs + buf * BN * ROWB + (wn * (BN / 2) + lr) * ROWB + lh * 16;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint4 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *(const uint4*)(a + i * 32 * ROWB + s * 32);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = *(const uint4*)(b + j * 32 * ROWB + s * 32);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) Mma<TC>::run(af[i], bf[j], acc[i][j]);
    }
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue ---------------------------------------------------------------------------
  const long coff = (long)z0 * p.sC_z0 + (long)z1 * p.sC_z1;
  const float* R = p.R ? (p.r_lowp ? (const float*)((const uint16_t*)p.R + (long)z0 * p.sR_z0 + (long)z1 * p.sR_z1)
                                   : p.R + (long)z0 * p.sR_z0 + (long)z1 * p.sR_z1) : nullptr;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = m0 + wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
      if (row >= p.M) continue;
      const int bidx = row / p.rows_per_batch;
      long rrow = row;
      if (p.r_up) {
        int rem = row - bidx * HW;
        int y = rem / p.W, x = rem - y * p.W;
        rrow = ((long)bidx * (p.H >> 1) + (y >> 1)) * (p.W >> 1) + (x >> 1);
      }
      const float bm = p.bias_m ? p.bias_m[row] : 0.f;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * (BN / 2) + j * 32 + lr;
        if (col >= p.N) continue;
        float val = acc[i][j][v] + bm;
        if (p.bias_n) val += p.bias_n[col];
        if (p.bias_bn) val += p.bias_bn[(long)bidx * p.ld_bn + col];
        if (R) val += res_load1<TC>(R, rrow * p.ldr + col, p.r_lowp);
        val *= p.alpha;
        if (p.c_nchw) {
          const int pix = row - bidx * p.rows_per_batch;
          ((float*)p.C)[((long)bidx * p.N + col) * p.rows_per_batch + pix] = val * p.row_scale[bidx];
        } else if (p.c_f32) {
          ((float*)p.C)[coff + (long)row * p.ldc + col] = val;
        } else {
          ((TC*)p.C)[coff + (long)row * p.ldc + col] = from_f32<TC>(val);
        }
      }
    }
  }
}

template <typename TC, bool AF32, int BM, int BN>
static int launch_t(const GemmParams& p, hipStream_t stream) {
  constexpr int smem = 2 * (BM + BN) * ROWB;
  auto kern = gemm_kernel<TC, AF32, BM, BN>;
  T2P_TRY(ensure_dynamic_lds((const void*)kern, smem));
  dim3 grid((p.N + BN - 1) / BN, (p.M + BM - 1) / BM, p.nz0 * p.nz1);
  ProfScope prof;
  if (prof.on()) {
    prof_shape(prof.rec, p);
    prof.rec.flops = 2.0 * p.M * p.N * (double)p.taps * (p.C0 + p.C1) * p.nz0 * p.nz1;
    prof.rec.kind = p.taps == 9 ? 2 : 1;
  }
  T2P_TRY(prof.open(stream));
  hipLaunchKernelGGL(kern, grid, dim3(256), smem, stream, p);
  T2P_TRY(prof.close());
  prof.commit();
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

int num_cus() {
  static int n[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  if (!n[dev]) {
    hipDeviceProp_t prop;
    n[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return n[dev];
}

static bool dma_eligible(const GemmParams& p) {
  if (!g_plan.dma || p.dtype == DT_F32 || p.a_f32) return false;
  if (p.C0 % 64 != 0 || p.C1 % 64 != 0) return false;   // whole 64-channel K-tiles only (else v1)
  if (p.M < 128 || p.N < 64) return false;              // small problems: v1's 64x64 tiles fill the chip better
  if (p.a_up && p.taps != 9) return false;
  if (p.c_nchw) return false;
  if (((long)p.M + 256) * std::max(p.lda0, p.lda1) * 2 >= (1L << 31)) return false;   // 32-bit offset arithmetic
  if ((long)p.M + 512 >= (1L << 24) || std::max(p.lda0, p.lda1) * 2 >= (1L << 24)) return false;   // row * stride in one 24-bit multiply
  const long a_rows = (p.taps == 9 || p.a_up) ? (long)(p.M / (p.H * p.W)) * (p.a_up ? (p.H / 2) * (p.W / 2) : p.H * p.W) : p.M;
  const long lim = (1L << 31) - 64;
  if (a_rows * p.lda0 * 2 >= lim || (p.A1 && a_rows * p.lda1 * 2 >= lim)) return false;
  if ((long)p.N * p.ldb * 2 >= lim) return false;
  return true;
}

// Tile geometry (0: 256x128x3, 1: 256x256x2, 2: 128x128x2, 3: 512x128x2) and split-K factor of a launch (the switches: plan.h).
DmaPlan dma_plan(const GemmParams& p) {
  const long z = (long)p.nz0 * p.nz1;
  const int nk = ((p.C0 + p.C1 + 63) / 64) * p.taps + (p.CX0 + p.CX1) / 64;
  const bool can_split = p.ws && z == 1;
  auto fits = [&](int ns) { return (size_t)ns * p.M * p.N * 4 <= p.ws_bytes; };
  const long t256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256) * z;
  int geom;
  if (g_plan.dma_geom == 1) geom = 0;
  else if (g_plan.dma_geom == 2) geom = 2;
  else if (g_plan.dma_geom == 3) geom = 1;
  else if (g_plan.dma_geom == 4) geom = 3;
  else if (p.M < 256) geom = 2;
  else {
    // largest tile that still gives about one workgroup per CU: big tiles are 15-20 % more efficient
    // (860-1020 vs 710-830 TFLOP/s on the conv shapes), but a short problem spread over few
    // workgroups is latency-bound and finishes sooner with more, smaller tiles
    const long t128 = (long)((p.M + 255) / 256) * ((p.N + 127) / 128) * z;
    const long t512 = (long)((p.M + 511) / 512) * ((p.N + 127) / 128) * z;
    if (g_plan.dma_geom == 5) geom = (p.N >= 256 && p.N % 256 == 0) ? 1 : 0;   // former policy, kept for A/B
    else if (p.N % 256 == 0 && t256 >= 200) geom = 1;
    else if (g_plan.dma_geom != 6 && p.N <= 128 && t512 >= 200) geom = 3;      // narrow outputs: tall tile, same 128x64 wave tile
    else if (t128 >= 200) geom = 0;
    else if (g_plan.midsplit && g_plan.splitk && !g_plan.force_nsplit && can_split && p.N % 256 == 0 && t256 >= 48 && nk >= 32 &&
             std::min<long>(256 / t256, nk / 8) >= 2 && fits((int)std::min<long>(256 / t256, nk / 8))) {
      // long-K problem with 48..128 big tiles (conv at the 16x16 level of cfg2): the 128x128 geometry would
      // run one 4-wave workgroup per CU (320-470 TFLOP/s measured); 256x256 tiles with the K loop split so
      // that tiles x splits ~ 256 workgroups reach 570-770
      return {1, (int)std::min<long>(256 / t256, nk / 8)};
    }
    else geom = 2;
  }
  const int BM = geom == 2 ? 128 : (geom == 3 ? 512 : 256), BN = geom == 1 ? 256 : 128;
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  int nsplit = 1;
  if (g_plan.force_nsplit > 0) {
    if (can_split && g_plan.force_nsplit > 1 && nk >= 2 * g_plan.force_nsplit) nsplit = g_plan.force_nsplit;
  } else if (g_plan.splitk && can_split && tiles < g_plan.split_tiles && nk >= 16) {
    // the tile grid cannot fill the chip and the K loop is long (low-resolution levels)
    // (tiles x splits ~ one workgroup per CU: a target of 256 measured 0.2 ms per step better than 384 at cfg2 and cfg3,
    // 128 .. 192 and 320 .. 768 worse; at least 4 K-tiles per split, 2 .. 12 within noise)
    nsplit = std::min(std::min(nk / 4, (g_plan.split_target + tiles - 1) / tiles), 32);
  }
  while (nsplit > 1 && !fits(nsplit)) --nsplit;
  // 128 x 128 tiles on at most one workgroup per CU: such a launch is bound by the latency of its K-steps (0.47 us each with
  // the 2-stage ring: every step waits for the DMA issued one step earlier), so it takes the 4-stage ring (geometry 4: the
  // same tile with three K-tiles in flight, 128 KiB of LDS)
  if (geom == 2 && g_plan.deep_ring && (long)tiles * nsplit * z <= num_cus()) geom = 4;
  return {geom, nsplit};
}
bool gemm_can_fuse_shortcut(const GemmParams& p) {
  return g_plan.fuse_shortcut && dma_eligible(p) && p.taps == 9 && !p.a_up;
}
static bool dma_uses_splitk(const GemmParams& p) { return dma_plan(p).nsplit > 1; }
static int dma_pick_geom(const GemmParams& p) { return dma_plan(p).geom; }

// the second pass can apply a following GroupNorm: split-K launch whose samples are blocks of <= 256 rows, whole groups per
// 64-column slab, no per-chunk column statistics wanted on top
bool gemm_fuses_post_gn(const GemmParams& p, int groups) {
  if (!g_plan.post_gn || !dma_eligible(p) || p.nz0 * p.nz1 != 1 || p.dtype == DT_F32 || !dma_uses_splitk(p) || !splitk_reduce_vec_ok(p)) return false;
  const int HW = p.rows_per_batch;
  if (HW < 1 || HW > 256 || p.M % HW != 0 || p.bias_m || p.c_nchw || (p.col_stats && HW % 64 != 0)) return false;
  if (p.r_up && (HW != p.H * p.W)) return false;
  if (groups <= 0 || p.N % 64 != 0 || p.N % groups != 0 || 64 % (p.N / groups) != 0) return false;
  return true;
}

// true when launch_gemm(p) with p.geglu set will apply the fused GEGLU epilogue
bool gemm_fuses_geglu(const GemmParams& p) {
  if (!dma_eligible(p) || p.nz0 * p.nz1 != 1 || p.c_f32 || p.R || p.bias_bn || p.bias_m) return false;
  if (p.N % 4 != 0 || p.ldc % 2 != 0) return false;
  return !dma_uses_splitk(p);
}

// true when launch_gemm(p) will run the LDS-DMA kernel without split-K and with a vector
// epilogue, i.e. when a non-null p.col_stats will be filled
// same with a compute-dtype (16-bit) output: statistics are still taken from the fp32 values
bool gemm_fuses_col_stats_lowp(const GemmParams& p) {
  GemmParams q = p;
  q.c_f32 = 1;
  return !p.c_f32 && p.dtype != DT_F32 && gemm_fuses_col_stats(q);
}

bool gemm_fuses_col_stats(const GemmParams& p) {
  if (!dma_eligible(p) || p.nz0 * p.nz1 != 1 || !p.c_f32) return false;
  if (p.N % 4 != 0 || p.ldc % 4 != 0 || (p.R && p.ldr % 4 != 0) || (p.bias_bn && p.ld_bn % 4 != 0)) return false;
  if (dma_uses_splitk(p) && !splitk_reduce_vec_ok(p)) return false;   // scalar second pass: no statistics
  return p.M % 64 == 0;
}

// GemmParams::c_frag: a plain product on the 256 x 256 register-epilogue kernel, 16-bit output, whole 32-row x 32-column fragments
bool gemm_writes_frag_major(const GemmParams& p) {
  if (!dma_eligible(p) || p.taps != 1 || p.c_f32 || p.geglu || p.col_stats || p.gn_out || p.r_up || p.c_nchw) return false;
  if (g_plan.dma_ring != 2 || g_plan.dma_geom != 0) return false;
  const DmaPlan plan = dma_plan(p);
  if (plan.geom != 1 || plan.nsplit != 1 || !reg_epilogue_ok(p, 1, 0)) return false;
  if (p.frag_col0 < 0 || p.frag_col0 % 64 != 0 || (p.N - p.frag_col0) % 32 != 0 || p.frag_ns != (p.N - p.frag_col0) / 32) return false;
  if (p.rows_per_batch > 1 ? (p.rows_per_batch % 32 != 0 || p.M % p.rows_per_batch != 0 || p.nz0 * p.nz1 != 1) : (p.M % 32 != 0 || p.nz1 != 1)) return false;
  return true;
}

template <typename TC>
static int launch_dma(const GemmParams& p, hipStream_t stream) {
  if (p.taps == 9) return p.a_up ? launch_dma_mode<TC, 2>(p, stream) : launch_dma_mode<TC, 1>(p, stream);
  return launch_dma_mode<TC, 0>(p, stream);
}

template <typename TC, bool AF32>
static int launch_tile(const GemmParams& p, hipStream_t stream) {
  // small problems: 64x64 tiles give more workgroups and waste less on ragged edges
  const long tiles128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128) * p.nz0 * p.nz1;
  if (p.N <= 64 || p.M <= 64 || tiles128 < 128) return launch_t<TC, AF32, 64, 64>(p, stream);
  return launch_t<TC, AF32, 128, 128>(p, stream);
}

// true when launch_gemm(p) will take the thin-output kernel
static bool thin_conv_eligible(const GemmParams& p) {
  if (p.dtype == DT_F32 || p.a_f32 || p.taps != 9 || p.a_up || !p.c_nchw || !p.c_f32) return false;
  if (p.A1 || p.R || p.bias_m || p.bias_bn || p.nz0 * p.nz1 != 1 || p.alpha != 1.f || p.geglu) return false;
  if (p.N > 8 || (p.C0 != 32 && p.C0 != 64 && p.C0 != 128 && p.C0 != 256) || p.lda0 != p.C0) return false;
  return p.rows_per_batch == p.H * p.W && p.M % (p.H * p.W) == 0;
}

bool gemm_applies_a_norm(const GemmParams& p) { return g_plan.thin_conv && g_plan.a_norm && thin_conv_eligible(p) && p.C0 <= 256; }

// launch_gemm takes the row-resident kernel (rowgemm.hip), given its copy of the weights: switch 49 at 2: wherever it is eligible; at 1:
// from 128 workgroups of 128 rows on, and where the plan it replaces is the 256 x 256 16x16x32 kernel, whose bits it reproduces
bool gemm_rowres_planned(const GemmParams& p) {
  if (!g_plan.rowres || g_plan.dbg || !dma_eligible(p) || !gemm_rowres_eligible(p)) return false;
  const DmaPlan plan = dma_plan(p);
  if (plan.nsplit != 1) return false;
  return g_plan.rowres == 2 || (p.M / 128 >= 128 && plan.geom == 1 && g_plan.dma_ring == 2);
}

int launch_gemm(const GemmParams& p, hipStream_t stream) {
  const int vec = p.dtype == DT_F32 ? 4 : 8;
  const int Ctot = p.C0 + p.C1;
  T2P_REQUIRE(p.A0 && p.Bw && (p.C || p.gn_out), "null operand");
  if (p.gn_out) {
    GemmParams q = p;
    q.gn_out = nullptr; q.gn_gamma = q.gn_beta = nullptr;
    T2P_REQUIRE(p.gn_gamma && p.gn_beta && gemm_fuses_post_gn(q, p.gn_groups), "a following GroupNorm rides only on the split-K second pass (ask gemm_fuses_post_gn)");
  }
  T2P_REQUIRE(p.M > 0 && p.N > 0 && Ctot > 0, "empty problem");
  T2P_REQUIRE(p.taps == 1 || p.taps == 9, "taps must be 1 or 9");
  T2P_REQUIRE(p.dtype != DT_F32 || p.a_f32, "fp32 compute takes fp32 sources");
  T2P_REQUIRE(!p.r_lowp || (p.R && p.dtype != DT_F32), "a 16-bit residual needs a 16-bit compute dtype");
  T2P_REQUIRE(p.lda0 % vec == 0 && p.ldb % vec == 0, "row strides must be multiples of the 16-byte vector");
  T2P_REQUIRE(p.lda0 >= ((p.C0 + vec - 1) / vec) * vec, "lda0 too small");
  T2P_REQUIRE(p.ldb >= (long)(p.taps - 1) * Ctot + ((Ctot + vec - 1) / vec) * vec, "ldb too small");
  if (p.A1) {
    T2P_REQUIRE(p.C0 % vec == 0 && p.lda1 % vec == 0 && p.C1 % vec == 0, "concat sources must be vector aligned");
    T2P_REQUIRE(p.nz0 * p.nz1 == 1, "batched GEMM takes a single A source");
  } else {
    T2P_REQUIRE(p.C1 == 0, "C1 without A1");
  }
  if (p.taps == 9) T2P_REQUIRE(Ctot % vec == 0, "3x3 convolution needs channels % vector == 0");
  if (p.taps == 9 || p.a_up || p.r_up || p.c_nchw) {
    T2P_REQUIRE(p.H > 0 && p.W > 0 && p.M % (p.H * p.W) == 0, "spatial mode needs H, W with M = batch*H*W");
    T2P_REQUIRE(p.nz0 * p.nz1 == 1, "spatial modes are not batched");
  }
  if (p.a_up || p.r_up) T2P_REQUIRE(p.H % 2 == 0 && p.W % 2 == 0, "up-sampling needs even H, W");
  if (p.r_up || p.c_nchw) T2P_REQUIRE(p.rows_per_batch == p.H * p.W, "rows_per_batch must be H*W");
  T2P_REQUIRE(p.rows_per_batch > 0, "rows_per_batch");
  T2P_REQUIRE(!p.c_nchw || (p.row_scale && p.c_f32), "nchw store needs row_scale and fp32 output");
  T2P_REQUIRE(((uintptr_t)p.A0 % 16) == 0 && ((uintptr_t)p.Bw % 16) == 0 && ((uintptr_t)p.A1 % 16) == 0,
              "operands must be 16-byte aligned");
  T2P_REQUIRE((long)(p.M + 127) / 128 < 65536, "M too large for grid.y");
  if (p.X0 || p.X1 || p.CX0 || p.CX1) {
    GemmParams q = p;
    q.X0 = q.X1 = nullptr; q.CX0 = q.CX1 = 0;
    T2P_REQUIRE(p.X0 && p.CX0 > 0 && p.CX0 % 64 == 0 && p.CX1 % 64 == 0 && (p.X1 != nullptr) == (p.CX1 > 0), "shortcut segment: whole 64-channel K-tiles");
    T2P_REQUIRE(gemm_can_fuse_shortcut(q), "shortcut segment: only on the LDS-DMA 3x3 convolution (ask gemm_can_fuse_shortcut)");
    T2P_REQUIRE(((uintptr_t)p.X0 % 16) == 0 && ((uintptr_t)p.X1 % 16) == 0 && p.ldx0 % 8 == 0 && p.ldx1 % 8 == 0, "shortcut segment: 16-byte aligned rows");
    T2P_REQUIRE(((long)p.M + 512) * std::max(p.ldx0, p.ldx1) * 2 < (1L << 31) - 64 && std::max(p.ldx0, p.ldx1) * 2 < (1L << 24), "shortcut segment: 32-bit offsets");
    T2P_REQUIRE(p.ldb >= 9L * (p.C0 + p.C1) + p.CX0 + p.CX1, "shortcut segment: weight rows hold 9 (C0 + C1) + CX0 + CX1 columns");
  }
  if (p.an_stats) {
    GemmParams q = p;
    q.an_stats = nullptr;
    T2P_REQUIRE(p.an_gamma && p.an_beta && p.an_groups > 0 && p.C0 % p.an_groups == 0 && gemm_applies_a_norm(q),
                "a GroupNorm of the A operand rides only on the thin-output head convolution (ask gemm_applies_a_norm)");
  }
  if (g_plan.thin_conv && thin_conv_eligible(p)) {
    // the head convolution: timed as "conv on the register-staged kernel" by the profile hooks' kind 2
    ProfScope prof;
    if (prof.on()) {
      prof_shape(prof.rec, p);
      prof.rec.flops = 2.0 * p.M * p.N * 9.0 * p.C0; prof.rec.kind = 2;
    }
    T2P_TRY(prof.open(stream));
    const int rc = launch_thin_conv(p, stream);
    T2P_TRY(prof.close());
    prof.commit();
    return rc;
  }
  if (p.Bw_rf && gemm_rowres_planned(p)) {
    // the K = 512 projections on the row-resident kernel (rowgemm.hip): same results as the 256 x 256 plan, bit for bit
    ProfScope prof;
    if (prof.on()) {
      prof_shape(prof.rec, p);
      prof.rec.flops = 2.0 * p.M * p.N * (double)p.C0; prof.rec.kind = 1; prof.rec.name = gemm_rowres_kernel_name(p.dtype);
      prof.rec.bytes = (double)p.M * p.C0 * 2 + (double)p.N * p.C0 * 2 + (double)p.M * (p.geglu ? p.N / 2 : p.N) * 2 + (p.R ? (double)p.M * p.N * 2 : 0.0);
    }
    T2P_TRY(prof.open(stream));
    const int rc = launch_gemm_rowres(p, stream);
    T2P_TRY(prof.close());
    prof.commit();
    return rc;
  }
  if (dma_eligible(p)) return p.dtype == DT_BF16 ? launch_dma<bf16_t>(p, stream) : launch_dma<f16_t>(p, stream);
  switch (p.dtype) {
    case DT_F32: return launch_tile<float, true>(p, stream);
    case DT_BF16: return p.a_f32 ? launch_tile<bf16_t, true>(p, stream) : launch_tile<bf16_t, false>(p, stream);
    case DT_F16: return p.a_f32 ? launch_tile<f16_t, true>(p, stream) : launch_tile<f16_t, false>(p, stream);
  }
  set_last_error("launch_gemm: unknown dtype");
  return T2P_ERR_INVALID;
}

}  // namespace t2p
