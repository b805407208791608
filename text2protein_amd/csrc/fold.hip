// Restraint-free fold: decoded 6D maps -> N / CA / C per residue, and the reference's restraint score.
//
// The maps fix the backbone without an energy function: Cb-Cb distances under the cut-off give the Cb trace (geodesic completion,
// classical MDS, stress refinement on the known pairs); phi gives the direction CA - Cb of every residue, theta the azimuth of N about
// it, and the featuriser's own virtual-Cb identity (dataset.py:409) then fixes C.  The mirror image is told apart by chain closure.
// Input is what t2p_op_decode_6d writes: absval [B][4][L*L] whose first n*n entries per channel are the row-major (n, n) map,
// n = lengths[b] (-1 = improper mask).  Dist and omega are read from the upper triangle (load_constraints' np.triu,
// rosetta_min/utils.py:140,157), theta and phi per ordered pair.
//
// Five launches on the caller's stream, nothing read back between them:
//   fold_embed_kernel     one workgroup per chain: Floyd-Warshall over the known distances (matrix in LDS up to 128 residues, in a
//                         global / L2 scratch matrix above), double centring, three leading eigenpairs by subspace iteration with a
//                         Cholesky re-orthonormalisation, then the stress steps with the coordinates in LDS
//   fold_frames_kernel    one wavefront per residue (the chains spread over ceil(L / 4) x B workgroups): both hands' N / CA / C
//   fold_finish_kernel    one workgroup per chain: residues without a frame placed, closure of both hands, the hand kept, xyz
//   restraint_rows_kernel one workgroup per map row (L x B): the four harmonic sums of that row, in double
//   restraint_final_kernel  the rows of a chain summed in row order
// Every reduction is a fixed butterfly over the lanes followed by a sum over the waves in wave order (wave_reduce.h), every loop over
// residues runs in index order: two calls give the same bits, and a chain gives the same bits whatever batch or padding it sits in.
// The vectors, the virtual Cb, the ideal backbone, the angle and the dihedral are backbone_geom.h's, shared with refine.hip.
#include "backbone_geom.h"
#include "t2p_common.h"
#include "t2p_kernels.h"
#include "wave_reduce.h"

namespace t2p {
namespace {

constexpr int FOLD_THREADS = 1024;      // fold_embed_kernel: 16 wavefronts
constexpr int FOLD_WAVES = FOLD_THREADS / 64;
constexpr int FOLD_LANES = 8;           // lanes that share one residue's gradient in a stress step
constexpr int FOLD_ROUND = FOLD_THREADS / FOLD_LANES;
constexpr int FOLD_MDS_ITERS = 100;     // subspace iterations: the error falls by (lambda_4 / lambda_3) per step and the stress steps
                                        // that follow start from the result, so it need not be tight
constexpr float FOLD_UNREACHED = 1.0e30f;
constexpr float FOLD_DMAX = 20.f;       // an encoded far pair decodes to exactly this
constexpr float FOLD_NEIGHBOUR = 12.f;  // the reference's restraint filter (rosetta_min/utils.py:137)

using namespace geom;        // V3 / F3 / D3, the virtual Cb, the ideal backbone, the dihedrals (backbone_geom.h)

__device__ __forceinline__ bool proper_length(int n, int L) { return n >= 1 && n <= L; }
// the symmetric distance of a pair: the upper-triangle entry
__device__ __forceinline__ float pair_dist(const float* dmap, int n, int i, int j) { return i < j ? dmap[(long)i * n + j] : dmap[(long)j * n + i]; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Cb trace of one chain.  M is the (n, n) work matrix with row stride n: geodesics, then the centred Gram matrix, then the known
// distances again (-1 unknown, -2 diagonal) for the stress steps.  info[b] = {stress rms, unreachable pairs, lambda_1..3}.
template <bool IN_LDS>
__global__ __launch_bounds__(FOLD_THREADS) void fold_embed_kernel(const float* __restrict__ absval, const int* __restrict__ lengths, int L,
                                                                  float known_below, int stress_steps, float* gmat,
                                                                  float* __restrict__ cb_out, float* __restrict__ info) {
  extern __shared__ float dyn_mat[];
  __shared__ float red[FOLD_WAVES * 9];
  __shared__ float xs[2][FOLD_MAX_L * 3];       // coordinates, two copies (Jacobi steps); V and W of the subspace iteration before that
  __shared__ float rowmean[FOLD_MAX_L];
  __shared__ int degree[FOLD_MAX_L];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = lengths[b];
  float* out = info + (long)b * 8;
  if (!proper_length(n, L)) {                       // uniform over the workgroup
    if (t < 8) out[t] = 0.f;
    return;
  }
  float* M = IN_LDS ? dyn_mat : gmat + (long)b * L * L;
  const float* dmap = absval + (long)b * 4 * L * L;
  const int nn = n * n;
  // 1. known pairs
  for (int e = t; e < nn; e += FOLD_THREADS) {
    const int i = e / n, j = e - i * n;
    const float d = pair_dist(dmap, n, i, j);
    M[e] = i == j ? 0.f : (d < known_below ? d : FOLD_UNREACHED);
  }
  __syncthreads();
  // 2. geodesics.  In step k row k and column k keep their values (M[k][k] = 0), so the update is safe in place.
  for (int k = 0; k < n; ++k) {
    for (int e = t; e < nn; e += FOLD_THREADS) {
      const int i = e / n, j = e - i * n;
      M[e] = fminf(M[e], M[i * n + k] + M[k * n + j]);
    }
    __syncthreads();
  }
  float longest = 0.f, unreached[1] = {0.f};
  for (int e = t; e < nn; e += FOLD_THREADS) {
    const float v = M[e];
    if (v < 0.5f * FOLD_UNREACHED) longest = fmaxf(longest, v);
    else unreached[0] += 1.f;
  }
  longest = wave_max(longest);
  if (lane == 0) rowmean[wave] = longest;
  __syncthreads();
  for (int q = 0; q < FOLD_WAVES; ++q) longest = fmaxf(longest, rowmean[q]);
  block_sum<1, FOLD_WAVES>(unreached, red);
  // 3. double centring of the squared geodesics (a pair in another component sits DMAX beyond the longest geodesic)
  for (int e = t; e < nn; e += FOLD_THREADS) {
    const float v = M[e] < 0.5f * FOLD_UNREACHED ? M[e] : longest + FOLD_DMAX;
    M[e] = v * v;
  }
  __syncthreads();
  for (int i = wave; i < n; i += FOLD_WAVES) {
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += M[i * n + j];
    s = wave_sum(s);
    if (lane == 0) rowmean[i] = s / (float)n;
  }
  __syncthreads();
  float total[1] = {0.f};
  for (int i = t; i < n; i += FOLD_THREADS) total[0] += rowmean[i];
  block_sum<1, FOLD_WAVES>(total, red);
  const float grand = total[0] / (float)n;
  for (int e = t; e < nn; e += FOLD_THREADS) {
    const int i = e / n, j = e - i * n;
    M[e] = -0.5f * (M[e] - rowmean[i] - rowmean[j] + grand);
  }
  // 4. three leading eigenpairs: V <- orth(M V).  The iteration finds the eigenvalues of largest MAGNITUDE; classical MDS wants the
  // algebraically largest, so each axis is scaled by its Rayleigh quotient v^T M v, sign included: an axis whose eigenvalue is negative
  // (possible only for distances no point set has) is dropped (scaled by sqrt(1e-12)), not embedded with sqrt(|lambda|)
  float* V = xs[0];
  float* W = xs[1];
  for (int e = t; e < 3 * n; e += FOLD_THREADS) {
    const unsigned h = (unsigned)e * 2654435761u + 0x9e3779b9u;
    V[e] = (float)((h >> 8) & 0xffffu) * (1.f / 65536.f) - 0.5f;
  }
  __syncthreads();
  float lambda[3] = {0.f, 0.f, 0.f};
  for (int it = 0; it < FOLD_MDS_ITERS; ++it) {
    for (int i = wave; i < n; i += FOLD_WAVES) {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int j = lane; j < n; j += 64) {
        const float m = M[i * n + j];
        s0 += m * V[3 * j]; s1 += m * V[3 * j + 1]; s2 += m * V[3 * j + 2];
      }
      s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
      if (lane == 0) { W[3 * i] = s0; W[3 * i + 1] = s1; W[3 * i + 2] = s2; }
    }
    __syncthreads();
    float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};        // W^T W: 00 01 02 11 12 22, then v_c . (M v_c)
    for (int i = t; i < n; i += FOLD_THREADS) {
      const float a = W[3 * i], c = W[3 * i + 1], d = W[3 * i + 2];
      g[0] += a * a; g[1] += a * c; g[2] += a * d; g[3] += c * c; g[4] += c * d; g[5] += d * d;
      g[6] += a * V[3 * i]; g[7] += c * V[3 * i + 1]; g[8] += d * V[3 * i + 2];
    }
    block_sum<9, FOLD_WAVES>(g, red);
    const float r00 = sqrtf(fmaxf(g[0], 1e-30f));
    const float r01 = g[1] / r00, r02 = g[2] / r00;
    const float r11 = sqrtf(fmaxf(g[3] - r01 * r01, 1e-12f * g[3] + 1e-30f));
    const float r12 = (g[4] - r01 * r02) / r11;
    const float r22 = sqrtf(fmaxf(g[5] - r02 * r02 - r12 * r12, 1e-12f * g[5] + 1e-30f));
    for (int i = t; i < n; i += FOLD_THREADS) {
      const float v0 = W[3 * i] / r00;
      const float v1 = (W[3 * i + 1] - v0 * r01) / r11;
      const float v2 = (W[3 * i + 2] - v0 * r02 - v1 * r12) / r22;
      V[3 * i] = v0; V[3 * i + 1] = v1; V[3 * i + 2] = v2;
    }
    lambda[0] = g[6]; lambda[1] = g[7]; lambda[2] = g[8];       // of the V this step started from: orthonormal from step 1 on
    __syncthreads();
  }
  // the sign of an eigenvector is arbitrary: every axis is made to rise along the chain, which names the two hands
  float corr[3] = {0.f, 0.f, 0.f};
  for (int i = t; i < n; i += FOLD_THREADS) {
    const float r = (float)i - 0.5f * (float)(n - 1);
    corr[0] += r * V[3 * i]; corr[1] += r * V[3 * i + 1]; corr[2] += r * V[3 * i + 2];
  }
  block_sum<3, FOLD_WAVES>(corr, red);
  for (int e = t; e < 3 * n; e += FOLD_THREADS) {
    const int c = e % 3;
    const float x = V[e] * (corr[c] < 0.f ? -1.f : 1.f) * sqrtf(fmaxf(lambda[c], 1e-12f));
    V[e] = isfinite(x) ? x : 0.f;
  }
  // 5. stress refinement on the known pairs
  for (int e = t; e < nn; e += FOLD_THREADS) {
    const int i = e / n, j = e - i * n;
    const float d = pair_dist(dmap, n, i, j);
    M[e] = i == j ? -2.f : (d < known_below ? d : -1.f);
  }
  __syncthreads();
  for (int i = wave; i < n; i += FOLD_WAVES) {
    int c = 0;
    for (int j = lane; j < n; j += 64) c += M[i * n + j] >= 0.f;
    c = wave_sum(c);
    if (lane == 0) degree[i] = max(c, 1);
  }
  __syncthreads();
  const int sub = t & (FOLD_LANES - 1), chunks = (n + FOLD_LANES - 1) / FOLD_LANES;       // chunks of eight j, all of them visited
  int cur = 0;
  for (int step = 0; step < stress_steps; ++step) {
    const float* X = xs[cur];
    float* Y = xs[cur ^ 1];
    for (int base = 0; base < n; base += FOLD_ROUND) {        // uniform trip count: the shuffles below need every lane
      const int i = base + t / FOLD_LANES;
      float gx = 0.f, gy = 0.f, gz = 0.f;
      if (i < n) {
        const float xi = X[3 * i], yi = X[3 * i + 1], zi = X[3 * i + 2];
        const int first = (i & (FOLD_LANES - 1)) % chunks;    // rotated start: the eight residues of a wave read different LDS banks
        for (int q = 0; q < chunks; ++q) {
          int c = q + first;                                  // first < chunks: one subtraction is the modulo
          if (c >= chunks) c -= chunks;
          const int j = c * FOLD_LANES + sub;
          if (j >= n) continue;
          const float d = M[i * n + j];
          if (d < -1.5f) continue;                            // the diagonal
          const float dx = xi - X[3 * j], dy = yi - X[3 * j + 1], dz = zi - X[3 * j + 2];
          const float r = sqrtf(dx * dx + dy * dy + dz * dz);
          float coef;
          if (d >= 0.f) coef = r - d;
          else if (r < FOLD_DMAX) coef = r - FOLD_DMAX;       // an unknown pair is at least DMAX apart
          else continue;
          coef /= fmaxf(r, 1e-6f);
          gx += coef * dx; gy += coef * dy; gz += coef * dz;
        }
      }
      lanes_sum<FOLD_LANES>(gx, gy, gz);
      if (i < n && sub == 0) {
        const float s = 0.5f / (float)degree[i];
        Y[3 * i] = X[3 * i] - s * gx; Y[3 * i + 1] = X[3 * i + 1] - s * gy; Y[3 * i + 2] = X[3 * i + 2] - s * gz;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  const float* X = xs[cur];
  float acc[2] = {0.f, 0.f};
  for (int e = t; e < nn; e += FOLD_THREADS) {
    const float d = M[e];
    if (d < 0.f) continue;
    const int i = e / n, j = e - i * n;
    const float dx = X[3 * i] - X[3 * j], dy = X[3 * i + 1] - X[3 * j + 1], dz = X[3 * i + 2] - X[3 * j + 2];
    const float r = sqrtf(dx * dx + dy * dy + dz * dz) - d;
    acc[0] += r * r; acc[1] += 1.f;
  }
  block_sum<2, FOLD_WAVES>(acc, red);
  for (int e = t; e < 3 * n; e += FOLD_THREADS) cb_out[(long)b * L * 3 + e] = isfinite(X[e]) ? X[e] : 0.f;
  if (t == 0) {
    const float rms = acc[1] > 0.f ? sqrtf(acc[0] / acc[1]) : 0.f;
    out[0] = isfinite(rms) ? rms : 0.f;
    out[1] = unreached[0];
    for (int c = 0; c < 3; ++c) out[2 + c] = isfinite(lambda[c]) ? lambda[c] : 0.f;
    out[5] = out[6] = out[7] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// N / CA / C of one residue about its Cb, for both hands.  frames [B][2][L][9], bad [B][2][L].
// Hand 1 is the mirror z -> -z of the Cb trace.  The normal equations of the direction u are mirror-symmetric (u_1 = S u_0), so they
// are solved once; the azimuth is not: with a = -u the CA -> Cb axis and w the part of the neighbour direction orthogonal to a, the
// direction of N about a is  w cos(theta) - (a x w) sin(theta)  (get_dihedrals' sign, dataset.py:364-380), and mirroring flips the
// sign of the cross product, so hand 1 is S (sum w cos + sum (a x w) sin).
__global__ __launch_bounds__(256) void fold_frames_kernel(const float* __restrict__ absval, const int* __restrict__ lengths, int L, float known_below,
                                                          const float* __restrict__ cb, float* __restrict__ frames, int* __restrict__ bad) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = lengths[b];
  if (!proper_length(n, L) || i >= n) return;               // uniform over the wavefront
  const float* maps = absval + (long)b * 4 * L * L;
  const float* dmap = maps;
  const float* theta = maps + 2L * L * L;
  const float* phi = maps + 3L * L * L;
  const float* X = cb + (long)b * L * 3;
  const F3 ci = load3<float>(X + 3 * i);
  float s[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // A: xx xy xz yy yz zz, rhs x y z, count
  for (int j = lane; j < n; j += 64) {
    const float d = pair_dist(dmap, n, i, j);
    if (j == i || !(d < known_below) || !(d <= FOLD_NEIGHBOUR)) continue;
    F3 e = load3<float>(X + 3 * j) - ci;
    e = (1.f / fmaxf(sqrtf(dot(e, e)), 1e-6f)) * e;
    const float cp = cosf(phi[(long)i * n + j]);
    s[0] += e.x * e.x; s[1] += e.x * e.y; s[2] += e.x * e.z; s[3] += e.y * e.y; s[4] += e.y * e.z; s[5] += e.z * e.z;
    s[6] += e.x * cp; s[7] += e.y * cp; s[8] += e.z * cp; s[9] += 1.f;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) s[k] = wave_sum(s[k]);
  // the symmetric 3x3 solve by cofactors
  const float c00 = s[3] * s[5] - s[4] * s[4], c01 = s[2] * s[4] - s[1] * s[5], c02 = s[1] * s[4] - s[2] * s[3];
  const float c11 = s[0] * s[5] - s[2] * s[2], c12 = s[1] * s[2] - s[0] * s[4], c22 = s[0] * s[3] - s[1] * s[1];
  const float det = s[0] * c00 + s[1] * c01 + s[2] * c02, tr = (s[0] + s[3] + s[5]) * (1.f / 3.f);
  bool fail = s[9] < 2.5f || !(det >= 1e-4f * tr * tr * tr) || !(det > 0.f);
  F3 u = {0.f, 0.f, 1.f};
  if (!fail) {
    u = (1.f / det) * F3{c00 * s[6] + c01 * s[7] + c02 * s[8], c01 * s[6] + c11 * s[7] + c12 * s[8], c02 * s[6] + c12 * s[7] + c22 * s[8]};
    const float un = sqrtf(dot(u, u));
    if (!(un >= 1e-3f) || !isfinite(un)) { fail = true; u = {0.f, 0.f, 1.f}; }
    else u = (1.f / un) * u;
  }
  const F3 a = -1.f * u;
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};               // sum w cos(theta), sum (a x w) sin(theta)
  for (int j = lane; j < n; j += 64) {
    const float d = pair_dist(dmap, n, i, j);
    if (j == i || !(d < known_below) || !(d <= FOLD_NEIGHBOUR)) continue;
    F3 e = load3<float>(X + 3 * j) - ci;
    e = (1.f / fmaxf(sqrtf(dot(e, e)), 1e-6f)) * e;
    F3 w = e - dot(e, a) * a;
    const float wn = sqrtf(dot(w, w));
    if (!(wn >= 1e-3f)) continue;
    w = (1.f / wn) * w;
    float st, ct;
    sincosf(theta[(long)i * n + j], &st, &ct);
    const F3 aw = cross(a, w);
    v[0] += ct * w.x; v[1] += ct * w.y; v[2] += ct * w.z; v[3] += st * aw.x; v[4] += st * aw.y; v[5] += st * aw.z;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
  if (lane != 0) return;
  for (int h = 0; h < 2; ++h) {
    const float m = h ? -1.f : 1.f;                           // S = diag(1, 1, m)
    F3 p = h ? F3{v[0] + v[3], v[1] + v[4], -(v[2] + v[5])} : F3{v[0] - v[3], v[1] - v[4], v[2] - v[5]};
    const float pn = sqrtf(dot(p, p));
    const bool bad_h = fail || !(pn >= 1e-3f) || !isfinite(pn);
    float* f = frames + (((long)b * 2 + h) * L + i) * 9;
    bad[((long)b * 2 + h) * L + i] = bad_h ? 1 : 0;
    if (bad_h) {
      for (int k = 0; k < 9; ++k) f[k] = 0.f;
      continue;
    }
    p = (1.f / pn) * p;
    const F3 cbh = {ci.x, ci.y, m * ci.z}, uh = {u.x, u.y, m * u.z}, ah = -1.f * uh;
    const F3 ca = cbh + R_CB_F * uh;
    const F3 nn = ca + BOND_N_CA_F * (COS_NCACB_F * ah + SIN_NCACB_F * p);
    // C from the identity, linear in c: (K3 I + K1 [b]x) c = (Cb - CA) - K2 b, and
    // (alpha I + beta [b]x)^-1 = (alpha^2 I - alpha beta [b]x + beta^2 b b^T) / (alpha (alpha^2 + beta^2 |b|^2))
    const F3 bv = ca - nn, r = (cbh - ca) - K2_F * bv;
    const float den = K3_F * (K3_F * K3_F + K1_F * K1_F * dot(bv, bv));
    const F3 c = (1.f / den) * ((K3_F * K3_F) * r - (K3_F * K1_F) * cross(bv, r) + (K1_F * K1_F * dot(bv, r)) * bv);
    store3(f, nn); store3(f + 3, ca); store3(f + 6, ca + c);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Per chain: residues without a frame take the offsets (atom - Cb) of the nearest framed residue before them, else after them, else
// fixed ones; closure of both hands; the hand kept; xyz, status, placed and the first diagnostics.
// diag [B][16] double: hand, closure of hand 0 / 1, stress rms, 4 scores, 4 counts (restraint_final_kernel), unreachable pairs, lambda_1..3.
__global__ __launch_bounds__(256) void fold_finish_kernel(const int* __restrict__ lengths, int L, const float* __restrict__ cb,
                                                          float* __restrict__ frames, const int* __restrict__ bad, const float* __restrict__ info,
                                                          float* __restrict__ xyz, int* __restrict__ status, unsigned char* __restrict__ placed,
                                                          double* __restrict__ diag) {
  __shared__ float red[4 * 4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = lengths[b];
  float* out = xyz + (long)b * L * 9;
  double* dg = diag + (long)b * 16;
  if (!proper_length(n, L)) {
    for (int e = t; e < L * 9; e += 256) out[e] = 0.f;
    for (int e = t; e < L; e += 256) placed[(long)b * L + e] = 0;
    if (t < 16) dg[t] = 0.0;
    if (t == 0) status[b] = -1;
    return;
  }
  const float* X = cb + (long)b * L * 3;
  for (int e = t; e < 2 * n; e += 256) {
    const int h = e / n, i = e - h * n;
    const int* bh = bad + ((long)b * 2 + h) * L;
    if (!bh[i]) continue;
    int k = i - 1;
    while (k >= 0 && bh[k]) --k;
    if (k < 0) {
      k = i + 1;
      while (k < n && bh[k]) ++k;
    }
    float* f = frames + (((long)b * 2 + h) * L + i) * 9;
    const float m = h ? -1.f : 1.f;
    const F3 ci = {X[3 * i], X[3 * i + 1], m * X[3 * i + 2]};
    if (k >= n) {
      store3(f, ci + F3{-1.2f, -0.9f, 0.f}); store3(f + 3, ci + F3{0.f, -R_CB_F, 0.f}); store3(f + 6, ci + F3{1.25f, -0.9f, 0.f});
    } else {
      const float* g = frames + (((long)b * 2 + h) * L + k) * 9;      // a framed residue: never written here
      const F3 ck = {X[3 * k], X[3 * k + 1], m * X[3 * k + 2]};
      for (int q = 0; q < 3; ++q) store3(f + 3 * q, ci + (load3<float>(g + 3 * q) - ck));
    }
  }
  __syncthreads();
  float s[4] = {0.f, 0.f, 0.f, 0.f};                          // closure sums of hand 0 / 1, residues placed in hand 0 / 1
  for (int i = t; i < n; i += 256)
    for (int h = 0; h < 2; ++h) {
      const float* f = frames + (((long)b * 2 + h) * L + i) * 9;
      if (i + 1 < n) {
        const F3 d = load3<float>(f + 6) - load3<float>(f + 9);
        s[h] += fabsf(sqrtf(dot(d, d)) - BOND_C_N_F);
      }
      s[2 + h] += (float)bad[((long)b * 2 + h) * L + i];
    }
  block_sum<4, 4>(s, red);
  const float c0 = n > 1 ? s[0] / (float)(n - 1) : 0.f, c1 = n > 1 ? s[1] / (float)(n - 1) : 0.f;
  const int hand = c0 <= c1 ? 0 : 1;
  float broken[1] = {0.f};
  const float* f = frames + ((long)b * 2 + hand) * L * 9;
  for (int e = t; e < L * 9; e += 256) {
    float x = e < n * 9 ? f[e] : 0.f;
    if (!isfinite(x)) { x = 0.f; broken[0] += 1.f; }
    out[e] = x;
  }
  for (int e = t; e < L; e += 256) placed[(long)b * L + e] = e < n ? (unsigned char)bad[((long)b * 2 + hand) * L + e] : 0;
  block_sum<1, 4>(broken, red);
  if (t == 0) {
    const float* in = info + (long)b * 8;
    const bool ok = in[1] == 0.f && s[2 + hand] == 0.f && broken[0] == 0.f && isfinite(c0) && isfinite(c1);
    status[b] = ok ? 0 : 1;
    dg[0] = hand; dg[1] = isfinite(c0) ? c0 : 0.0; dg[2] = isfinite(c1) ? c1 : 0.0; dg[3] = in[0];
    dg[12] = in[1]; dg[13] = in[2]; dg[14] = in[3]; dg[15] = in[4];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The restraint score, load_constraints' sets (rosetta_min/utils.py:119-206) with the harmonic forms Rosetta applies, in double:
//   dist   i < j, 0 < d <= 12                 ((|Cb_i - Cb_j| - d) / dist_std)^2
//   omega  i < j, omega != 0, d <= 12         circular, dihedral CA_i Cb_i Cb_j CA_j
//   theta  a != b, d[a][b] <= 12              circular, dihedral N_a CA_a Cb_a Cb_b
//   phi    the same pairs                     harmonic, angle CA_a Cb_a Cb_b
// with Cb the virtual Cb of the given backbone.  The filter reads d[a][b] as stored, not symmetrised, as the reference does.
__device__ __forceinline__ void residue_atoms(const float* r, D3& nn, D3& ca, D3& cbeta) {
  nn = load3<double>(r); ca = load3<double>(r + 3);
  const D3 bv = ca - nn, cv = load3<double>(r + 6) - ca;
  cbeta = ca + cb_offset(bv, cv);
}

__global__ __launch_bounds__(128) void restraint_rows_kernel(const float* __restrict__ xyz, const float* __restrict__ absval,
                                                             const int* __restrict__ lengths, int L, double inv_dist_std, double inv_angle_std,
                                                             double* __restrict__ rows) {
  __shared__ double red[2 * 8];
  const int b = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
  const int n = lengths[b];
  if (!proper_length(n, L) || i >= n) return;               // uniform over the workgroup; such rows are never read
  const float* maps = absval + (long)b * 4 * L * L;
  const long LL = (long)L * L;
  const float* R = xyz + (long)b * L * 9;
  D3 ni, cai, cbi;
  residue_atoms(R + 9 * i, ni, cai, cbi);
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};                   // four sums, four counts
  for (int j = t; j < n; j += 128) {
    if (j == i) continue;
    const long e = (long)i * n + j;
    const double d = maps[e];
    if (!(d <= (double)FOLD_NEIGHBOUR)) continue;
    D3 nj, caj, cbj;
    residue_atoms(R + 9 * j, nj, caj, cbj);
    const D3 dv = cbj - cbi;
    const double r = sqrt(dot(dv, dv));
    double term;
    if (i < j && d > 0.0) {
      term = (r - d) * inv_dist_std;
      term *= term;
      s[0] += isfinite(term) ? term : 0.0; s[4] += 1.0;
    }
    const double om = maps[LL + e];
    if (i < j && om != 0.0) {
      term = wrap_angle(dihedral_or_zero(cai, cbi, cbj, caj) - om) * inv_angle_std;
      term *= term;
      s[1] += isfinite(term) ? term : 0.0; s[5] += 1.0;
    }
    term = wrap_angle(dihedral_or_zero(ni, cai, cbi, cbj) - (double)maps[2 * LL + e]) * inv_angle_std;
    term *= term;
    s[2] += isfinite(term) ? term : 0.0; s[6] += 1.0;
    term = (angle(cai, cbi, cbj) - (double)maps[3 * LL + e]) * inv_angle_std;
    term *= term;
    s[3] += isfinite(term) ? term : 0.0; s[7] += 1.0;
  }
  block_sum<8, 2>(s, red);
  if (t < 8) rows[((long)b * L + i) * 8 + t] = s[t];
}

// out[b * stride + 0..7] = the four sums and the four counts of chain b, the rows added in row order
__global__ __launch_bounds__(64) void restraint_final_kernel(const int* __restrict__ lengths, int L, const double* __restrict__ rows,
                                                             double* __restrict__ out, int stride) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= 8) return;
  const int n = lengths[b];
  double s = 0.0;
  if (proper_length(n, L))
    for (int i = 0; i < n; ++i) s += rows[((long)b * L + i) * 8 + t];
  out[(long)b * stride + t] = s;
}

struct FoldWorkspace {            // byte offsets into the caller's workspace (WorkspaceCarve)
  size_t cb, frames, bad, info, rows, mat, total;
  FoldWorkspace(int B, int L) {
    WorkspaceCarve w;
    cb = w.take((size_t)B * L * 3 * 4);
    frames = w.take((size_t)B * 2 * L * 9 * 4);
    bad = w.take((size_t)B * 2 * L * 4);
    info = w.take((size_t)B * 8 * 4);
    rows = w.take((size_t)B * L * 8 * 8);
    mat = w.take(L > FOLD_LDS_MAX ? (size_t)B * L * L * 4 : 0);
    total = w.total;
  }
};

}  // namespace

long fold6d_workspace_bytes(int B, int L) {
  if (B <= 0 || L <= 0 || L > FOLD_MAX_L) return -1;
  return (long)FoldWorkspace(B, L).total;
}

int launch_restraint_score(const float* xyz, const float* absval, const int* lengths, int B, int L, float dist_std, float angle_std_deg,
                           double* out, int stride, void* workspace, long workspace_bytes, hipStream_t s) {
  T2P_REQUIRE(xyz && absval && lengths && out && workspace && B > 0 && L > 0, "restraint_score arguments");
  T2P_REQUIRE(L <= FOLD_MAX_L && B <= 65535 && stride >= 8, "restraint_score: map or batch too large");
  T2P_REQUIRE(dist_std > 0.f && angle_std_deg > 0.f, "restraint_score: the standard deviations must be positive");
  const FoldWorkspace ws(B, L);
  T2P_REQUIRE(workspace_bytes >= (long)ws.total, "restraint_score: workspace smaller than t2p_op_fold_ws(batch, L)");
  double* rows = (double*)((char*)workspace + ws.rows);
  hipLaunchKernelGGL(restraint_rows_kernel, dim3(L, B), dim3(128), 0, s, xyz, absval, lengths, L, 1.0 / (double)dist_std,
                     1.0 / ((double)angle_std_deg * DEG), rows);
  T2P_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(restraint_final_kernel, dim3(B), dim3(64), 0, s, lengths, L, rows, out, stride);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

int launch_fold6d(const float* absval, const int* lengths, int B, int L, float known_below, int stress_steps, float dist_std, float angle_std_deg,
                  float* xyz, int* status, unsigned char* placed, double* diag, void* workspace, long workspace_bytes, hipStream_t s) {
  T2P_REQUIRE(absval && lengths && xyz && status && placed && diag && workspace && B > 0 && L > 0, "fold_6d arguments");
  T2P_REQUIRE(L <= FOLD_MAX_L && B <= 65535, "fold_6d: at most " + std::to_string(FOLD_MAX_L) + " residues and 65535 chains");
  T2P_REQUIRE(known_below > 0.f && stress_steps >= 0 && stress_steps <= 100000, "fold_6d: known_below must be positive, stress_steps in [0, 100000]");
  T2P_REQUIRE(dist_std > 0.f && angle_std_deg > 0.f, "fold_6d: the standard deviations must be positive");
  const FoldWorkspace ws(B, L);
  T2P_REQUIRE(workspace_bytes >= (long)ws.total, "fold_6d: workspace smaller than t2p_op_fold_ws(batch, L)");
  char* w = (char*)workspace;
  float* cb = (float*)(w + ws.cb);
  float* frames = (float*)(w + ws.frames);
  int* bad = (int*)(w + ws.bad);
  float* info = (float*)(w + ws.info);
  if (L <= FOLD_LDS_MAX) {
    const int lds = L * L * 4;
    T2P_TRY(ensure_dynamic_lds((const void*)fold_embed_kernel<true>, lds));
    hipLaunchKernelGGL(fold_embed_kernel<true>, dim3(B), dim3(FOLD_THREADS), lds, s, absval, lengths, L, known_below, stress_steps,
                       (float*)nullptr, cb, info);
  } else {
    hipLaunchKernelGGL(fold_embed_kernel<false>, dim3(B), dim3(FOLD_THREADS), 0, s, absval, lengths, L, known_below, stress_steps,
                       (float*)(w + ws.mat), cb, info);
  }
  T2P_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fold_frames_kernel, dim3((L + 3) / 4, B), dim3(256), 0, s, absval, lengths, L, known_below, cb, frames, bad);
  T2P_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fold_finish_kernel, dim3(B), dim3(256), 0, s, lengths, L, cb, frames, bad, info, xyz, status, placed, diag);
  T2P_HIP_CHECK(hipGetLastError());
  return launch_restraint_score(xyz, absval, lengths, B, L, dist_std, angle_std_deg, diag + 4, 16, workspace, workspace_bytes, s);
}

}  // namespace t2p
