#include "gemm_device.h"

namespace t2p {

// ---- thin-output 3x3 convolution: the network head (nf -> 5 or 8 channels, NCHW fp32 x row scale) ----------
// As a GEMM this layer has N = 5: the 64-wide tile of the register-staged kernel spends 92 % of its MFMAs on
// padding and re-reads every input pixel nine times from L2 (426 us at cfg2 against a ~55 us HBM bound).  Here
// a workgroup owns an 8 x 16 pixel tile: the 10 x 18 halo of 16-bit input pixels is staged once in LDS (chunk
// index XOR pixel index: conflict-free 16-byte fragment reads), the <= 8 weight rows too, and each wavefront
// runs v_mfma_f32_16x16x32 on two rows of 16 pixels with the 16 MFMA columns holding the output channels.
struct ThinConvArgs {
  const void* x; const void* w; const float* bias; const float* row_scale; float* out;
  int B, H, W, Cin, Cout;
  long ldw;
  // optional: x is the raw map; act(GroupNorm(x)) is applied while the halo is staged (out.0 + out.1 of the head, ncsnpp.py:211-216)
  const float* gn_stats; const float* gn_gamma; const float* gn_beta;
  int gn_groups, gn_silu;
};

template <typename TC, int CH>   // CH: channels staged per pass (32, 64 or 128)
__global__ __launch_bounds__(512) void thin_conv_kernel(const ThinConvArgs a) {
  constexpr int TH = 8, TW = 16, WP = TW + 2, NPIX = (TH + 2) * WP;
  constexpr int cb = CH * 2, nchunk = CH / 8;               // bytes / 16-byte chunks per staged pixel
  constexpr int wrow = 9 * cb + 16;                         // padded weight row: lanes of a fragment read hit distinct banks
  constexpr int sw = (nchunk < 8 ? nchunk : 8) - 1;         // swizzle mask: stays inside the pixel's own chunks
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float nsc[256], nsh[256];                      // per-channel scale / shift of the fused GroupNorm (Cin <= 256)
  unsigned char* halo = smem;
  unsigned char* wl = smem + NPIX * cb;
  const int tid = threadIdx.x;
  const int tiles_x = (a.W + TW - 1) / TW, tiles_y = (a.H + TH - 1) / TH;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const bool norm = a.gn_stats != nullptr;
  if (norm) {
    // the same arithmetic as the separate GroupNorm-apply pass (gn_apply16_kernel): y = x * (rstd gamma) + (beta - mean rstd gamma)
    if (tid < a.Cin) {
      const int g = tid / (a.Cin / a.gn_groups);
      const float mean = a.gn_stats[2 * (b * a.gn_groups + g)], rstd = a.gn_stats[2 * (b * a.gn_groups + g) + 1];
      const float sc = rstd * a.gn_gamma[tid];
      nsc[tid] = sc;
      nsh[tid] = a.gn_beta[tid] - mean * sc;
    }
    __syncthreads();
  }
  const int x0 = tx * TW, y0 = ty * TH;
  const TC* xb = (const TC*)a.x + (long)b * a.H * a.W * a.Cin;
  const int wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;   // wave = pixel row of the tile
  const bool colv = r < a.Cout;                             // MFMA column = output channel
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < a.Cin; c0 += CH) {                  // channel passes: 58 KiB of LDS at CH = 128 -> two blocks per CU
    if (c0) __syncthreads();                                // the previous pass is no longer read
    for (int i = tid; i < NPIX * nchunk; i += 512) {
      const int P = i / nchunk, j = i - P * nchunk;
      const int gy = y0 + P / WP - 1, gx = x0 + P % WP - 1;
      u32x4_t v = {0u, 0u, 0u, 0u};                         // zero padding outside the map (of the NORMALISED map: stays zero)
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        v = *(const u32x4_t*)(xb + ((long)gy * a.W + gx) * a.Cin + c0 + j * 8);
        if (norm) {
          union { u32x4_t u; TC e[8]; } in, o;
          in.u = v;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int c = c0 + j * 8 + e;
            float y = to_f32(in.e[e]) * nsc[c] + nsh[c];
            if (a.gn_silu) y = y * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(y * -1.44269504088896341f));
            o.e[e] = from_f32<TC>(y);
          }
          v = o.u;
        }
      }
      *(u32x4_t*)(halo + P * cb + (((j & ~sw) | ((j ^ P) & sw)) << 4)) = v;
    }
    for (int i = tid; i < a.Cout * 9 * nchunk; i += 512) {
      const int co = i / (9 * nchunk), k = i - co * 9 * nchunk, tap = k / nchunk, j = k - tap * nchunk;
      *(u32x4_t*)(wl + co * wrow + k * 16) = *(const u32x4_t*)((const TC*)a.w + (long)co * a.ldw + (long)tap * a.Cin + c0 + j * 8);
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap % 3;
      const int P = (wave + dy) * WP + r + dx;
      u32x4_t af[CH / 32], bf[CH / 32];                     // one tap's fragments in flight before its MFMAs (<= 128 VGPRs
#pragma unroll                                               //  in total: two 512-thread blocks per CU)
      for (int kc = 0; kc < CH / 32; ++kc) {
        const int j = kc * 4 + g;
        af[kc] = *(const u32x4_t*)(halo + P * cb + (((j & ~sw) | ((j ^ P) & sw)) << 4));
        bf[kc] = (u32x4_t){0u, 0u, 0u, 0u};
        if (colv) bf[kc] = *(const u32x4_t*)(wl + r * wrow + (tap * nchunk + j) * 16);
      }
#pragma unroll
      for (int kc = 0; kc < CH / 32; ++kc) Mma16<TC>::run(af[kc], bf[kc], acc);
    }
  }
  if (!colv) return;
  // 16x16 accumulator: column = lane & 15 (channel), row = (lane >> 4) * 4 + register (pixel of the row)
  const int y = y0 + wave;
  if (y >= a.H) return;
  const float bias = a.bias ? a.bias[r] : 0.f, sc = a.row_scale ? a.row_scale[b] : 1.f;
  float* o = a.out + (((long)b * a.Cout + r) * a.H + y) * a.W;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int x = x0 + g * 4 + v;
    if (x < a.W) o[x] = (acc[v] + bias) * sc;
  }
}

template <typename TC, int CH>
static int launch_thin_conv_ch(const ThinConvArgs& a, hipStream_t stream) {
  constexpr int smem = 180 * CH * 2 + 8 * (9 * CH * 2 + 16);
  const int tiles = ((a.W + 15) / 16) * ((a.H + 7) / 8);
  hipLaunchKernelGGL((thin_conv_kernel<TC, CH>), dim3((unsigned)((long)a.B * tiles)), dim3(512), smem, stream, a);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

template <typename TC>
static int launch_thin_conv_t(const GemmParams& p, hipStream_t stream) {
  ThinConvArgs a;
  a.x = p.A0; a.w = p.Bw; a.bias = p.bias_n; a.row_scale = p.row_scale; a.out = (float*)p.C;
  a.B = p.M / (p.H * p.W); a.H = p.H; a.W = p.W; a.Cin = p.C0; a.Cout = p.N; a.ldw = p.ldb;
  a.gn_stats = p.an_stats; a.gn_gamma = p.an_gamma; a.gn_beta = p.an_beta; a.gn_groups = p.an_groups; a.gn_silu = p.an_silu;
  if (p.C0 == 32) return launch_thin_conv_ch<TC, 32>(a, stream);
  if (p.C0 == 64) return launch_thin_conv_ch<TC, 64>(a, stream);
  return launch_thin_conv_ch<TC, 128>(a, stream);           // 128 or 256 channels: one or two passes
}
int launch_thin_conv(const GemmParams& p, hipStream_t stream) {
  return p.dtype == DT_BF16 ? launch_thin_conv_t<bf16_t>(p, stream) : launch_thin_conv_t<f16_t>(p, stream);
}

}  // namespace t2p
