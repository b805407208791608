// Secondary structure from CA traces: P-SEA (Labesse et al. 1997) with its published thresholds, the annotation the
// reference asks biotite for (dataset.py:121-123) and the source of the three `ss` channels and of ss_indices.
//
// One workgroup of 256 threads per chain, one launch, nothing read back.  The CA trace (double, 12 KB at 512 residues) and the
// per-residue flags stay in LDS; every thread strides over the residues.  Five phases with a barrier between them:
//   load      CA of every residue inside the length, its presence flag, the finite / 1e6 check
//   measure   d2, d3, d4, r and a of every residue in double -> the four flag bits; the contact count of every potential-strand residue
//             (a loop over the whole trace in LDS)
//   cores     the thread of a run's first residue walks the run: helix cores (>= 5), strand cores (>= 5, or 3..4 with >= 5 contacts
//             summed in index order), one extension residue per end judged on its own flag bit (no cascade)
//   letters   c, then a, then b, c again for a residue without a CA; the per-letter and agreement counts
//   runs      the thread of a letter run's first residue counts it when it holds at least 4 residues (encode.sse_blocks' blocks)
// Only integers are counted and only integer LDS atomics add them, so two calls give the same bits; tests/sse_oracle.py is the same
// text in numpy and the GPU test asks for equality.
#include "backbone_geom.h"
#include "t2p_common.h"
#include "t2p_kernels.h"

namespace t2p {
namespace {

constexpr int SSE_THREADS = 256;
constexpr double SSE_MAX_COORD = 1.0e6;
enum : unsigned char { SSE_PH = 1, SSE_PS = 2, SSE_HEXT = 4, SSE_SEXT = 8 };

__device__ inline bool within(double v, double lo, double hi) { return v >= lo && v <= hi; }      // false for NaN

__global__ __launch_bounds__(SSE_THREADS) void annotate_sse_kernel(const float* __restrict__ xyz, const int* __restrict__ len,
                                                                   const unsigned char* __restrict__ atom_ok, int L, int atoms,
                                                                   const unsigned char* __restrict__ target,
                                                                   unsigned char* __restrict__ letters, int* __restrict__ counts,
                                                                   int* __restrict__ status) {
  __shared__ double px[SSE_MAX_L], py[SSE_MAX_L], pz[SSE_MAX_L];
  __shared__ int contacts[SSE_MAX_L];
  __shared__ unsigned char has[SSE_MAX_L], flags[SSE_MAX_L], helix[SSE_MAX_L], strand[SSE_MAX_L], letter[SSE_MAX_L];
  __shared__ int cnt[12];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = len[b];
  unsigned char* out = letters + (size_t)b * L;
  if (n < 1 || n > L) {                                   // uniform over the workgroup
    for (int i = tid; i < L; i += SSE_THREADS) out[i] = 0;
    if (tid < 12) counts[b * 12 + tid] = 0;
    if (tid == 0) status[b] = -1;
    return;
  }
  if (tid < 12) cnt[tid] = 0;
  if (tid == 0) bad = 0;
  __syncthreads();

  // ---- load ----
  const int ca = atoms == 3 ? 1 : 0;
  for (int i = tid; i < n; i += SSE_THREADS) {
    const size_t at = ((size_t)b * L + i) * atoms + ca;
    bool ok = atom_ok ? atom_ok[at] != 0 : true;
    double x = 0.0, y = 0.0, z = 0.0;
    if (ok) {
      x = (double)xyz[at * 3], y = (double)xyz[at * 3 + 1], z = (double)xyz[at * 3 + 2];
      if (!(fabs(x) <= SSE_MAX_COORD && fabs(y) <= SSE_MAX_COORD && fabs(z) <= SSE_MAX_COORD)) {     // NaN fails the test too
        ok = false;
        x = y = z = 0.0;
        bad = 1;                                          // every writer stores the same value
      }
    }
    px[i] = x, py[i] = y, pz[i] = z;
    has[i] = ok;
    helix[i] = strand[i] = 0;
  }
  __syncthreads();

  // ---- measure ----
  for (int i = tid; i < n; i += SSE_THREADS) {
    const double nan = __builtin_nan("");
    double d2 = nan, d3 = nan, d4 = nan, r = nan, a = nan;
    const bool m1 = i >= 1 && has[i - 1], p0 = has[i], p1 = i + 1 < n && has[i + 1], p2 = i + 2 < n && has[i + 2], p3 = i + 3 < n && has[i + 3];
    if (m1) {
      const double ax = px[i - 1], ay = py[i - 1], az = pz[i - 1];
      if (p1) d2 = sqrt((ax - px[i + 1]) * (ax - px[i + 1]) + (ay - py[i + 1]) * (ay - py[i + 1]) + (az - pz[i + 1]) * (az - pz[i + 1]));
      if (p2) d3 = sqrt((ax - px[i + 2]) * (ax - px[i + 2]) + (ay - py[i + 2]) * (ay - py[i + 2]) + (az - pz[i + 2]) * (az - pz[i + 2]));
      if (p3) d4 = sqrt((ax - px[i + 3]) * (ax - px[i + 3]) + (ay - py[i + 3]) * (ay - py[i + 3]) + (az - pz[i + 3]) * (az - pz[i + 3]));
      if (p0 && p1) {
        const double ux = ax - px[i], uy = ay - py[i], uz = az - pz[i];
        const double vx = px[i + 1] - px[i], vy = py[i + 1] - py[i], vz = pz[i + 1] - pz[i];
        const double c = (ux * vx + uy * vy + uz * vz) / (sqrt(ux * ux + uy * uy + uz * uz) * sqrt(vx * vx + vy * vy + vz * vz));
        if (c == c) r = acos(fmin(1.0, fmax(-1.0, c))) * geom::RAD;                 // coincident CAs: 0 / 0, r stays undefined
        if (p2) {
          const double b0x = -ux, b0y = -uy, b0z = -uz, b1x = vx, b1y = vy, b1z = vz;
          const double b2x = px[i + 2] - px[i + 1], b2y = py[i + 2] - py[i + 1], b2z = pz[i + 2] - pz[i + 1];
          const double n1x = b0y * b1z - b0z * b1y, n1y = b0z * b1x - b0x * b1z, n1z = b0x * b1y - b0y * b1x;
          const double n2x = b1y * b2z - b1z * b2y, n2y = b1z * b2x - b1x * b2z, n2z = b1x * b2y - b1y * b2x;
          const double mx = n1y * n2z - n1z * n2y, my = n1z * n2x - n1x * n2z, mz = n1x * n2y - n1y * n2x;
          a = atan2((mx * b1x + my * b1y + mz * b1z) / sqrt(b1x * b1x + b1y * b1y + b1z * b1z), n1x * n2x + n1y * n2y + n1z * n2z) * geom::RAD;
        }
      }
    }
    unsigned char f = 0;
    if ((within(d3, 4.8, 5.8) && within(d4, 5.8, 7.0)) || (within(r, 77.0, 101.0) && within(a, 30.0, 70.0))) f |= SSE_PH;
    if ((within(d2, 6.1, 7.3) && within(d3, 9.0, 10.8) && within(d4, 11.3, 13.5)) ||
        (within(r, 110.0, 138.0) && (within(a, -180.0, -125.0) || within(a, 145.0, 180.0))))
      f |= SSE_PS;
    if (within(d3, 4.8, 5.8) || within(r, 77.0, 101.0)) f |= SSE_HEXT;
    if (within(d3, 9.0, 10.8)) f |= SSE_SEXT;
    flags[i] = f;
    int c = 0;
    if ((f & SSE_PS) && p0) {                             // ordered pairs (i, j), j any residue with a CA; j = i is at distance 0
      const double x = px[i], y = py[i], z = pz[i];
      for (int j = 0; j < n; ++j) {
        const double d = sqrt((x - px[j]) * (x - px[j]) + (y - py[j]) * (y - py[j]) + (z - pz[j]) * (z - pz[j]));
        c += has[j] && within(d, 4.2, 5.2);
      }
    }
    contacts[i] = c;
  }
  __syncthreads();

  // ---- cores and their extensions ----
  for (int i = tid; i < n; i += SSE_THREADS) {
    const unsigned char f = flags[i], before = i > 0 ? flags[i - 1] : 0;
    if ((f & SSE_PH) && !(before & SSE_PH)) {
      int e = i;
      while (e + 1 < n && (flags[e + 1] & SSE_PH)) ++e;
      if (e - i + 1 >= 5) {
        for (int k = i; k <= e; ++k) helix[k] = 1;        // an extension of a neighbouring core may store the same 1 here
        if (i > 0 && (before & SSE_HEXT)) helix[i - 1] = 1;
        if (e + 1 < n && (flags[e + 1] & SSE_HEXT)) helix[e + 1] = 1;
      }
    }
    if ((f & SSE_PS) && !(before & SSE_PS)) {
      int e = i, sum = contacts[i];
      while (e + 1 < n && (flags[e + 1] & SSE_PS)) sum += contacts[++e];
      const int m = e - i + 1;
      if (m >= 5 || (m >= 3 && sum >= 5)) {
        for (int k = i; k <= e; ++k) strand[k] = 1;
        if (i > 0 && (before & SSE_SEXT)) strand[i - 1] = 1;
        if (e + 1 < n && (flags[e + 1] & SSE_SEXT)) strand[e + 1] = 1;
      }
    }
  }
  __syncthreads();

  // ---- letters and the per-residue counts ----
  int c_a = 0, c_b = 0, c_c = 0, t_a = 0, t_aa = 0, t_b = 0, t_bb = 0, no_ca = 0;
  for (int i = tid; i < L; i += SSE_THREADS) {
    unsigned char l = 0;
    if (i < n) {
      l = 'c';
      if (helix[i]) l = 'a';
      if (strand[i]) l = 'b';                             // the strand wins an overlap
      if (!has[i]) l = 'c', ++no_ca;
      letter[i] = l;
      c_a += l == 'a', c_b += l == 'b', c_c += l == 'c';
      if (target) {
        const unsigned char t = target[(size_t)b * L + i];
        t_a += t == 'a', t_aa += t == 'a' && l == 'a', t_b += t == 'b', t_bb += t == 'b' && l == 'b';
      }
    }
    out[i] = l;
  }
  if (c_a) atomicAdd(&cnt[0], c_a);
  if (c_b) atomicAdd(&cnt[1], c_b);
  if (c_c) atomicAdd(&cnt[2], c_c);
  if (t_a) atomicAdd(&cnt[5], t_a);
  if (t_aa) atomicAdd(&cnt[6], t_aa);
  if (t_b) atomicAdd(&cnt[7], t_b);
  if (t_bb) atomicAdd(&cnt[8], t_bb);
  if (no_ca) atomicAdd(&cnt[9], no_ca);
  __syncthreads();

  // ---- runs of at least four equal letters ----
  for (int i = tid; i < n; i += SSE_THREADS) {
    const unsigned char l = letter[i];
    if (l != 'c' && (i == 0 || letter[i - 1] != l)) {
      int e = i;
      while (e + 1 < n && letter[e + 1] == l) ++e;
      if (e - i + 1 >= 4) atomicAdd(&cnt[l == 'a' ? 3 : 4], 1);
    }
  }
  __syncthreads();
  if (tid < 12) counts[b * 12 + tid] = cnt[tid];
  if (tid == 0) status[b] = bad;
}

}  // namespace

int launch_annotate_sse(const float* xyz, const int* len, const unsigned char* atom_ok, int B, int L, int atoms, const unsigned char* target,
                        unsigned char* letters, int* counts, int* status, hipStream_t s) {
  T2P_REQUIRE(xyz && len && letters && counts && status, "annotate_sse: a required pointer is null (xyz, len, letters, counts, status)");
  T2P_REQUIRE(B > 0 && B <= 65535, "annotate_sse: the batch must hold 1 to 65535 chains, not " + std::to_string(B));
  T2P_REQUIRE(L >= 1 && L <= SSE_MAX_L, "annotate_sse: the padded length must lie in [1, " + std::to_string(SSE_MAX_L) + "], not " + std::to_string(L));
  T2P_REQUIRE(atoms == 1 || atoms == 3, "annotate_sse: atoms must be 1 (a CA trace) or 3 (N / CA / C), not " + std::to_string(atoms));
  hipLaunchKernelGGL(annotate_sse_kernel, dim3(B), dim3(SSE_THREADS), 0, s, xyz, len, atom_ok, L, atoms, target, letters, counts, status);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

}  // namespace t2p
