// Refinement of folded backbones against the reference's restraint set: a staged Cartesian L-BFGS on N / CA / C.
//
// The energy, in double throughout, on the chain's 9 n coordinates with Cb the featuriser's virtual Cb (K1 (b x c) + K2 b + K3 c + CA):
//   dist   i < j, 0 < d <= 12                       ((|Cb_i - Cb_j| - d) / dist_std)^2
//   omega  i < j, omega != 0, d <= 12               circular, dihedral CA_i Cb_i Cb_j CA_j
//   theta  a != b, d[a][b] <= 12                    circular, dihedral N_a CA_a Cb_a Cb_b
//   phi    the same pairs                           harmonic, angle CA_a Cb_a Cb_b
// -- the sets of restraint_rows_kernel (fold.hip), less the theta restraints whose target phi lies within arm_min of 0 or 180 degrees and
// the omega restraints for which phi_ij or phi_ji does (the dihedral's arm is then collinear with its axis) -- counted in a stage only
// for sep_lo <= |i - j| < sep_hi; plus, unstaged, bonds (sigma 0.02 A), the three backbone angles (3 degrees), peptide planarity
// (dihedral CA C N CA about 180, 6 degrees) and a CA-CA repulsion max(0, 3.8 - r)^2 at |i - j| >= 2.
//
// One workgroup per chain, one launch per call.  Coordinates, gradient, direction and the trial point with its gradient live in LDS, the
// L-BFGS history and the per-residue restraint lists in the workspace.  The lists are built once per call in two passes (count, prefix
// sum, fill in j order), so an evaluation never rescans the maps.  The gradient is gathered: eight lanes own a residue, walk its list,
// evaluate every term the residue takes part in -- (i, j) and (j, i) -- keep the share of their own residue and add it up by a fixed
// butterfly; the energy of a term is counted by the residue that owns it (the smaller index, or the first of an ordered pair).  No
// atomics, every reduction in a fixed order (wave_reduce.h), nothing depends on the batch position or the padding: two calls give the
// same bits.  Every loop has a fixed bound.  The virtual Cb, the angle and the dihedral's value are backbone_geom.h's: fold.hip scores
// with the same Cb and angle, refine_rounds.hip measures with the same angle and dihedral.
#include <algorithm>
#include <cmath>

#include "backbone_geom.h"
#include "t2p_common.h"
#include "t2p_kernels.h"
#include "wave_reduce.h"

namespace t2p {
namespace {

constexpr int REFINE_THREADS = 512;
constexpr int REFINE_WAVES = REFINE_THREADS / 64;
constexpr int REFINE_LANES = 8;          // lanes that share one residue's gradient
constexpr int REFINE_ROUND = REFINE_THREADS / REFINE_LANES;
constexpr int REFINE_HISTORY = 8;
constexpr int REFINE_MAX_TRIALS = 20;
constexpr double ARMIJO_C1 = 1e-4, GRAD_TOL = 1e-3, CURVATURE_EPS = 1e-10;
constexpr double NEIGHBOUR = 12.0;       // the reference's restraint filter (rosetta_min/utils.py:137)
using namespace geom;        // D3, GUARD, PI / DEG, K1..K3, the ideal bonds and ANGLE_N_CA_C, the dihedral and the angle (backbone_geom.h)
constexpr double BOND_SIGMA = 0.02;
constexpr double ANGLE_CA_C_N = 116.2, ANGLE_C_N_CA = 121.7, ANGLE_SIGMA = 3.0, PEPT_SIGMA = 6.0;
constexpr double REP_RADIUS = 3.8;
constexpr int REP_MIN_SEP = 2;

enum : int { HAS_DIST = 1, HAS_OMEGA = 2, HAS_THETA_IJ = 4, HAS_PHI_IJ = 8, HAS_THETA_JI = 16, HAS_PHI_JI = 32 };
struct Entry {                 // one partner j of a residue i: the targets of every restraint the pair carries, 32 bytes
  int j, flags;
  float d, omega, theta_ij, phi_ij, theta_ji, phi_ji;
};
struct Stage { int sep_lo, sep_hi, max_iter; double w_dist, w_ang, w_rep; };
struct Schedule { int count; Stage s[REFINE_MAX_STAGES]; };
struct Params { double inv_dist_std, inv_angle_std, arm_min; };        // arm_min in rad

// dihedral p0-p1-p2-p3 (geom::dihedral_guarded) and its gradient with respect to the four points
__device__ __forceinline__ double dihedral_grad(D3 p0, D3 p1, D3 p2, D3 p3, D3& d0, D3& d1, D3& d2, D3& d3) {
  const double val = dihedral_guarded(p0, p1, p2, p3);
  const D3 f = p0 - p1, g = p1 - p2, h = p3 - p2;
  const D3 a = cross(f, g), b = cross(h, g);
  const double gl = sqrt(fmax(dot(g, g), GUARD));
  const double aa = fmax(dot(a, a), GUARD), bb = fmax(dot(b, b), GUARD);
  d0 = (-gl / aa) * a;
  d3 = (gl / bb) * b;
  const D3 fa = (dot(f, g) / (aa * gl)) * a, hb = (dot(h, g) / (bb * gl)) * b;
  d1 = (fa - hb) - d0;
  d2 = (hb - fa) - d3;
  return val;
}
// angle at pb (geom::angle) and its gradient with respect to pa and pc (that of pb is minus their sum)
__device__ __forceinline__ double angle_grad(D3 pa, D3 pb, D3 pc, D3& ga, D3& gc) {
  D3 v, w, cr;
  double sn;
  const double val = angle(pa, pb, pc, v, w, cr, sn);
  ga = (1.0 / fmax(dot(v, v) * sn, GUARD)) * cross(v, cr);
  gc = (-1.0 / fmax(dot(w, w) * sn, GUARD)) * cross(w, cr);
  return val;
}
__device__ __forceinline__ double finite_or_zero(double x) { return isfinite(x) ? x : 0.0; }

__device__ __forceinline__ bool refinable(int n, int L) { return n >= 2 && n <= L; }

// The flags of the ordered pair (i, j), i != j, and its targets.
__device__ __forceinline__ Entry pair_entry(const float* maps, long LL, int n, int i, int j, double arm_min) {
  const int lo = min(i, j), hi = max(i, j);
  const long e_up = (long)lo * n + hi, e_ij = (long)i * n + j, e_ji = (long)j * n + i;
  const float* phi = maps + 3 * LL;
  Entry en;
  en.j = j;
  en.d = maps[e_up]; en.omega = maps[LL + e_up];
  en.theta_ij = maps[2 * LL + e_ij]; en.phi_ij = phi[e_ij];
  en.theta_ji = maps[2 * LL + e_ji]; en.phi_ji = phi[e_ji];
  const double p_ij = en.phi_ij, p_ji = en.phi_ji;
  const bool flat_ij = p_ij < arm_min || p_ij > PI - arm_min, flat_ji = p_ji < arm_min || p_ji > PI - arm_min;
  const bool near_up = (double)en.d <= NEIGHBOUR, near_ij = (double)maps[e_ij] <= NEIGHBOUR, near_ji = (double)maps[e_ji] <= NEIGHBOUR;
  int f = 0;
  if (near_up && en.d > 0.f) f |= HAS_DIST;
  if (near_up && en.omega != 0.f && !flat_ij && !flat_ji) f |= HAS_OMEGA;
  if (near_ij) f |= HAS_PHI_IJ | (flat_ij ? 0 : HAS_THETA_IJ);
  if (near_ji) f |= HAS_PHI_JI | (flat_ji ? 0 : HAS_THETA_JI);
  en.flags = f;
  return en;
}

// Per-residue restraint lists of one chain: offsets[0..n] and the entries of residue i at entries[offsets[i] .. offsets[i + 1]), in j
// order.  Two passes with exact counts; the capacity L (L - 1) per chain holds every pair.
__device__ void build_lists(const float* maps, int L, int n, double arm_min, int* offsets, Entry* entries) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long LL = (long)L * L;
  for (int i = wave; i < n; i += REFINE_WAVES) {
    int c = 0;
    for (int j = lane; j < n; j += 64)
      if (j != i) c += pair_entry(maps, LL, n, i, j, arm_min).flags != 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);      // not wave_sum(c): as a call it moves the generated code
    if (lane == 0) offsets[i + 1] = c;
  }
  __syncthreads();
  if (t == 0) {
    int at = 0;
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) { at += offsets[i + 1]; offsets[i + 1] = at; }
  }
  __syncthreads();
  for (int i = wave; i < n; i += REFINE_WAVES) {
    int at = offsets[i];
    for (int j0 = 0; j0 < n; j0 += 64) {                      // uniform over the wavefront
      const int j = j0 + lane;
      Entry en;
      en.flags = 0;
      if (j < n && j != i) en = pair_entry(maps, LL, n, i, j, arm_min);
      const unsigned long long has = __ballot(en.flags != 0);
      if (en.flags != 0) entries[at + __popcll(has & ((1ull << lane) - 1ull))] = en;
      at += __popcll(has);
    }
  }
  __syncthreads();
}

// One evaluation: the eight unweighted terms (the same bits in every thread) and the gradient of the weighted total into G.
// X, G: 9 n doubles; CB: 3 n doubles; red: REFINE_WAVES * 8 doubles -- all LDS.  X must be visible to the workgroup on entry; G is on exit.
__device__ void evaluate(const double* X, double* G, double* CB, double* red, int n, const int* offsets, const Entry* entries, const Stage& st,
                         const Params& pr, double (&terms)[8]) {
  const int t = threadIdx.x, sub = t & (REFINE_LANES - 1);
  for (int i = t; i < n; i += REFINE_THREADS) {
    const D3 nn = load3<double>(X + 9 * i), ca = load3<double>(X + 9 * i + 3), cc = load3<double>(X + 9 * i + 6);
    store3(CB + 3 * i, virtual_cb(nn, ca, cc));
  }
  __syncthreads();
  const double ca_coef = 2.0 * pr.inv_angle_std * st.w_ang, cd_coef = 2.0 * pr.inv_dist_std * st.w_dist;
#pragma unroll
  for (int k = 0; k < 8; ++k) terms[k] = 0.0;
  for (int base = 0; base < n; base += REFINE_ROUND) {        // uniform trip count: the shuffles below need every lane
    const int i = base + t / REFINE_LANES;
    D3 gN = {0, 0, 0}, gCA = {0, 0, 0}, gC = {0, 0, 0}, gCB = {0, 0, 0};
    if (i < n) {
      const D3 ni = load3<double>(X + 9 * i), cai = load3<double>(X + 9 * i + 3), ci = load3<double>(X + 9 * i + 6), cbi = load3<double>(CB + 3 * i);
      const int end = offsets[i + 1];
      for (int k = offsets[i] + sub; k < end; k += REFINE_LANES) {
        const Entry en = entries[k];
        const int j = en.j, sep = abs(i - j);
        if (sep < st.sep_lo || sep >= st.sep_hi) continue;
        const D3 nj = load3<double>(X + 9 * j), caj = load3<double>(X + 9 * j + 3), cbj = load3<double>(CB + 3 * j);
        const bool first = i < j;
        if (en.flags & HAS_DIST) {
          const D3 dv = cbi - cbj;
          const double r = sqrt(dot(dv, dv));
          const double res = finite_or_zero((r - (double)en.d) * pr.inv_dist_std);
          if (first) terms[0] += res * res;
          axpy(gCB, cd_coef * res / fmax(r, GUARD), dv);
        }
#pragma unroll 1
        for (int q = 0; q < 3; ++q) {                           // omega, theta_ij, theta_ji: one dihedral body
          const int need = q == 0 ? HAS_OMEGA : (q == 1 ? HAS_THETA_IJ : HAS_THETA_JI);
          if (!(en.flags & need)) continue;
          D3 p0, p1, p2, p3, d0, d1, d2, d3;
          double target;
          if (q == 0) {
            target = en.omega;
            if (first) { p0 = cai; p1 = cbi; p2 = cbj; p3 = caj; } else { p0 = caj; p1 = cbj; p2 = cbi; p3 = cai; }
          } else if (q == 1) { target = en.theta_ij; p0 = ni; p1 = cai; p2 = cbi; p3 = cbj; }
          else { target = en.theta_ji; p0 = nj; p1 = caj; p2 = cbj; p3 = cbi; }
          const double val = dihedral_grad(p0, p1, p2, p3, d0, d1, d2, d3);
          const double res = finite_or_zero(wrap_angle(val - target) * pr.inv_angle_std), c = ca_coef * res;
          if (q == 0) {
            if (first) { terms[1] += res * res; axpy(gCA, c, d0); axpy(gCB, c, d1); }
            else { axpy(gCA, c, d3); axpy(gCB, c, d2); }
          } else if (q == 1) { terms[2] += res * res; axpy(gN, c, d0); axpy(gCA, c, d1); axpy(gCB, c, d2); }
          else axpy(gCB, c, d3);
        }
        if (en.flags & HAS_PHI_IJ) {
          D3 ga, gc;
          const double val = angle_grad(cai, cbi, cbj, ga, gc);
          const double res = finite_or_zero((val - (double)en.phi_ij) * pr.inv_angle_std), c = ca_coef * res;
          terms[3] += res * res;
          axpy(gCA, c, ga); axpy(gCB, -c, ga + gc);
        }
        if (en.flags & HAS_PHI_JI) {
          D3 ga, gc;
          const double val = angle_grad(caj, cbj, cbi, ga, gc);
          const double res = finite_or_zero((val - (double)en.phi_ji) * pr.inv_angle_std);
          axpy(gCB, ca_coef * res, gc);
        }
      }
      // repulsion between CA atoms
      for (int j = sub; j < n; j += REFINE_LANES) {
        if (abs(i - j) < REP_MIN_SEP) continue;
        const D3 dv = cai - load3<double>(X + 9 * j + 3);
        const double r = sqrt(dot(dv, dv));
        if (!(r < REP_RADIUS)) continue;
        const double res = REP_RADIUS - r;
        if (i < j) terms[7] += res * res;
        axpy(gCA, -2.0 * st.w_rep * res / fmax(r, GUARD), dv);
      }
      // bonded terms: lane 0 the residue's own, lane 1 the link to the residue before, lane 2 the link to the residue after
      const double cb_coef = 2.0 / BOND_SIGMA, cang = 2.0 / (ANGLE_SIGMA * DEG), cpep = 2.0 / (PEPT_SIGMA * DEG);
      if (sub == 0) {
        D3 dv = ni - cai;
        double r = sqrt(dot(dv, dv)), res = (r - BOND_N_CA) / BOND_SIGMA;
        terms[4] += res * res;
        axpy(gN, cb_coef * res / fmax(r, GUARD), dv); axpy(gCA, -cb_coef * res / fmax(r, GUARD), dv);
        dv = cai - ci;
        r = sqrt(dot(dv, dv)); res = (r - BOND_CA_C) / BOND_SIGMA;
        terms[4] += res * res;
        axpy(gCA, cb_coef * res / fmax(r, GUARD), dv); axpy(gC, -cb_coef * res / fmax(r, GUARD), dv);
        D3 ga, gc;
        res = (angle_grad(ni, cai, ci, ga, gc) - ANGLE_N_CA_C * DEG) / (ANGLE_SIGMA * DEG);
        terms[5] += res * res;
        axpy(gN, cang * res, ga); axpy(gC, cang * res, gc); axpy(gCA, -cang * res, ga + gc);
      } else if ((sub == 1 && i > 0) || (sub == 2 && i + 1 < n)) {
        const bool mine = sub == 2;                           // residue i is the first of the link (a, a + 1): it owns the energy
        const int a = mine ? i : i - 1;
        const D3 caa = load3<double>(X + 9 * a + 3), ca_c = load3<double>(X + 9 * a + 6), nb = load3<double>(X + 9 * a + 9), cab = load3<double>(X + 9 * a + 12);
        D3& gCAa = gCA; D3& gCa = gC;                         // a-side shares (kept when mine)
        D3& gNb = gN; D3& gCAb = gCA;                         // b-side shares (kept otherwise)
        D3 dv = ca_c - nb;
        double r = sqrt(dot(dv, dv)), res = (r - BOND_C_N) / BOND_SIGMA;
        if (mine) { terms[4] += res * res; axpy(gCa, cb_coef * res / fmax(r, GUARD), dv); }
        else axpy(gNb, -cb_coef * res / fmax(r, GUARD), dv);
        D3 ga, gc;
        res = (angle_grad(caa, ca_c, nb, ga, gc) - ANGLE_CA_C_N * DEG) / (ANGLE_SIGMA * DEG);
        if (mine) { terms[5] += res * res; axpy(gCAa, cang * res, ga); axpy(gCa, -cang * res, ga + gc); }
        else axpy(gNb, cang * res, gc);
        res = (angle_grad(ca_c, nb, cab, ga, gc) - ANGLE_C_N_CA * DEG) / (ANGLE_SIGMA * DEG);
        if (mine) { terms[5] += res * res; axpy(gCa, cang * res, ga); }
        else { axpy(gNb, -cang * res, ga + gc); axpy(gCAb, cang * res, gc); }
        D3 d0, d1, d2, d3;
        res = wrap_angle(dihedral_grad(caa, ca_c, nb, cab, d0, d1, d2, d3) - PI) / (PEPT_SIGMA * DEG);
        if (mine) { terms[6] += res * res; axpy(gCAa, cpep * res, d0); axpy(gCa, cpep * res, d1); }
        else { axpy(gNb, cpep * res, d2); axpy(gCAb, cpep * res, d3); }
      }
    }
    lanes_sum<REFINE_LANES>(gN.x, gN.y, gN.z, gCA.x, gCA.y, gCA.z, gC.x, gC.y, gC.z, gCB.x, gCB.y, gCB.z);
    if (i < n && sub == 0) {                                  // through the virtual Cb: Cb = CA + K1 (b x c) + K2 b + K3 c
      const D3 nn = load3<double>(X + 9 * i), ca = load3<double>(X + 9 * i + 3), cc = load3<double>(X + 9 * i + 6);
      const D3 bv = ca - nn, cv = cc - ca;
      const D3 gb = K1 * cross(cv, gCB) + K2 * gCB, gc = K1 * cross(gCB, bv) + K3 * gCB;
      store3(G + 9 * i, gN - gb); store3(G + 9 * i + 3, (gCA + gCB) + (gb - gc)); store3(G + 9 * i + 6, gC + gc);
    }
  }
  block_sum<8, REFINE_WAVES>(terms, red);
}
__device__ __forceinline__ double total_energy(const double (&t)[8], const Stage& st) {
  return st.w_dist * t[0] + st.w_ang * (t[1] + t[2] + t[3]) + t[4] + t[5] + t[6] + st.w_rep * t[7];
}

struct RefineWorkspace {          // byte offsets into the caller's workspace (WorkspaceCarve)
  size_t offsets, entries, history, total;
  RefineWorkspace(int B, int L) {
    WorkspaceCarve w;
    offsets = w.take((size_t)B * (L + 1) * 4);
    entries = w.take((size_t)B * L * (L > 1 ? L - 1 : 1) * sizeof(Entry));
    history = w.take((size_t)B * 2 * REFINE_HISTORY * 9 * L * 8);
    total = w.total;
  }
};
__host__ __device__ constexpr int refine_lds_bytes(int L) { return (5 * 9 * L + 3 * L + REFINE_WAVES * 8 + REFINE_HISTORY) * 8; }

// loads a chain into X as doubles; returns the number of non-finite coordinates (the same in every thread)
__device__ __forceinline__ double load_chain(const float* in, double* X, int n, double* red) {
  double bad[1] = {0.0};
  for (int e = threadIdx.x; e < 9 * n; e += REFINE_THREADS) {
    const float v = in[e];
    if (!isfinite(v)) bad[0] += 1.0;
    X[e] = (double)v;
  }
  block_sum<1, REFINE_WAVES>(bad, red);
  return bad[0];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One evaluation for given coordinates: out9 [B][9] = the eight unweighted terms and the weighted total, grad [B][L][3][3].
template <bool GROUPED>                                        // as refine_kernel's; grad may then be null
__global__ __launch_bounds__(REFINE_THREADS) void restraint_energy_kernel(const float* __restrict__ xyz, const float* __restrict__ absval,
                                                                          const int* __restrict__ lengths, int L, Stage st, Params pr,
                                                                          double* __restrict__ out9, double* __restrict__ grad, int* offsets_all,
                                                                          Entry* entries_all, int group) {
  extern __shared__ double lds[];
  double* X = lds;
  double* G = X + 9 * L;
  double* CB = G + 9 * L;
  double* red = CB + 3 * L;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = lengths[b];
  double* go = !GROUPED || grad ? grad + (long)b * L * 9 : nullptr;
  double terms[8];
  bool ok = refinable(n, L);                                   // uniform over the workgroup
  if (ok) ok = load_chain(xyz + (long)b * L * 9, X, n, red) == 0.0;
  if (!ok) {
    if (go)
      for (int e = t; e < 9 * L; e += REFINE_THREADS) go[e] = 0.0;
    if (t < 9) out9[(long)b * 9 + t] = 0.0;
    return;
  }
  int* offsets = offsets_all + (long)b * (L + 1);
  Entry* entries = entries_all + (long)b * L * (L - 1);
  build_lists(absval + (long)(GROUPED ? b / group : b) * 4 * L * L, L, n, pr.arm_min, offsets, entries);
  evaluate(X, G, CB, red, n, offsets, entries, st, pr, terms);
  if (go)
    for (int e = t; e < 9 * L; e += REFINE_THREADS) go[e] = e < 9 * n ? finite_or_zero(G[e]) : 0.0;
  if (t == 0) {
    for (int k = 0; k < 8; ++k) out9[(long)b * 9 + k] = finite_or_zero(terms[k]);
    out9[(long)b * 9 + 8] = finite_or_zero(total_energy(terms, st));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The staged L-BFGS of one chain.  Every vector operation is elementwise with element e owned by thread e mod REFINE_THREADS, so only
// the dot products and the evaluations synchronise.  GROUPED (refinement in rounds): workgroup b is a candidate with its
// own coordinates and its own entry of `lengths`, and reads the maps of chain b / group.  A template argument, not a run-time one: as
// live run-time scalars the two cost the plain kernel 4 % (more spills at 256 registers, measured), so <false> keeps the code it had.
template <bool GROUPED>
__global__ __launch_bounds__(REFINE_THREADS) void refine_kernel(const float* __restrict__ xyz_in, const float* __restrict__ absval,
                                                                const int* __restrict__ lengths, int L, Schedule sched, Params pr,
                                                                float* __restrict__ xyz_out, int* __restrict__ status, double* __restrict__ diag,
                                                                int* offsets_all, Entry* entries_all, double* history_all, int group) {
  extern __shared__ double lds[];
  double* X = lds;
  double* G = X + 9 * L;
  double* D = G + 9 * L;
  double* XT = D + 9 * L;
  double* GT = XT + 9 * L;
  double* CB = GT + 9 * L;
  double* red = CB + 3 * L;
  double* rho = red + REFINE_WAVES * 8;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = lengths[b];
  float* out = xyz_out + (long)b * L * 9;
  double* dg = diag + (long)b * 16;
  bool ok = refinable(n, L);
  int bad_status = -1;
  if (ok && load_chain(xyz_in + (long)b * L * 9, X, n, red) != 0.0) { ok = false; bad_status = 2; }
  if (!ok) {
    for (int e = t; e < 9 * L; e += REFINE_THREADS) out[e] = 0.f;
    if (t < 16) dg[t] = 0.0;
    if (t == 0) status[b] = bad_status;
    return;
  }
  const int nv = 9 * n;
  int* offsets = offsets_all + (long)b * (L + 1);
  Entry* entries = entries_all + (long)b * L * (L - 1);
  double* S = history_all + (long)b * 2 * REFINE_HISTORY * 9 * L;      // slot k at S + k * 9 L
  double* Y = S + (long)REFINE_HISTORY * 9 * L;
  const long slot = 9L * L;
  build_lists(absval + (long)(GROUPED ? b / group : b) * 4 * L * L, L, n, pr.arm_min, offsets, entries);

  double terms[8];
  const Stage last = sched.s[sched.count - 1];
  evaluate(X, G, CB, red, n, offsets, entries, last, pr, terms);
  const double e_start = total_energy(terms, last);
  int evals = 1, iters = 0, st_bits = 0, stages_done = 0;
  for (int si = 0; si < sched.count; ++si) {
    const Stage st = sched.s[si];
    evaluate(X, G, CB, red, n, offsets, entries, st, pr, terms);
    ++evals;
    double E = total_energy(terms, st), gamma = 1.0;
    int m = 0, head = 0;                                       // pairs held; the slot the next pair goes to
    for (int it = 0; it < st.max_iter; ++it) {
      double gg[1] = {0.0}, gmax = 0.0;
      for (int e = t; e < nv; e += REFINE_THREADS) { gg[0] += G[e] * G[e]; gmax = fmax(gmax, fabs(G[e])); }
      gmax = block_max<REFINE_WAVES>(gmax, red);
      block_sum<1, REFINE_WAVES>(gg, red);
      if (!(gmax >= GRAD_TOL)) break;
      bool steepest = m == 0;
      double gd = 0.0;
      if (!steepest) {                                         // two-loop recursion, q in D
        double alpha[REFINE_HISTORY];
        for (int e = t; e < nv; e += REFINE_THREADS) D[e] = G[e];
#pragma unroll
        for (int k = 0; k < REFINE_HISTORY; ++k) {
          if (k < m) {                                         // newest first
            const int idx = (head - 1 - k + 2 * REFINE_HISTORY) % REFINE_HISTORY;
            double sq[1] = {0.0};
            for (int e = t; e < nv; e += REFINE_THREADS) sq[0] += S[idx * slot + e] * D[e];
            block_sum<1, REFINE_WAVES>(sq, red);
            alpha[k] = rho[idx] * sq[0];
            for (int e = t; e < nv; e += REFINE_THREADS) D[e] -= alpha[k] * Y[idx * slot + e];
          }
        }
        for (int e = t; e < nv; e += REFINE_THREADS) D[e] *= gamma;
#pragma unroll
        for (int k = REFINE_HISTORY - 1; k >= 0; --k) {
          if (k < m) {                                         // oldest first
            const int idx = (head - 1 - k + 2 * REFINE_HISTORY) % REFINE_HISTORY;
            double yq[1] = {0.0};
            for (int e = t; e < nv; e += REFINE_THREADS) yq[0] += Y[idx * slot + e] * D[e];
            block_sum<1, REFINE_WAVES>(yq, red);
            const double c = alpha[k] - rho[idx] * yq[0];
            for (int e = t; e < nv; e += REFINE_THREADS) D[e] += c * S[idx * slot + e];
          }
        }
        double dd[1] = {0.0};
        for (int e = t; e < nv; e += REFINE_THREADS) { D[e] = -D[e]; dd[0] += G[e] * D[e]; }
        block_sum<1, REFINE_WAVES>(dd, red);
        gd = dd[0];
        if (!(gd < 0.0)) { steepest = true; m = 0; }
      }
      double step = 1.0;
      if (steepest) {
        for (int e = t; e < nv; e += REFINE_THREADS) D[e] = -G[e];
        gd = -gg[0];
        step = 1.0 / fmax(sqrt(gg[0]), 1.0);
      }
      ++iters;
      bool accepted = false;
      double Et = E;
      for (int trial = 0; trial < REFINE_MAX_TRIALS; ++trial) {
        for (int e = t; e < nv; e += REFINE_THREADS) XT[e] = X[e] + step * D[e];
        __syncthreads();
        evaluate(XT, GT, CB, red, n, offsets, entries, st, pr, terms);
        ++evals;
        Et = total_energy(terms, st);
        if (isfinite(Et) && Et <= E + ARMIJO_C1 * step * gd) { accepted = true; break; }
        step *= 0.5;
      }
      if (!accepted) {
        if (steepest) { st_bits |= 1; break; }
        m = 0;
        continue;
      }
      double d3[3] = {0.0, 0.0, 0.0};                          // s.y, s.s, y.y
      for (int e = t; e < nv; e += REFINE_THREADS) {
        const double s = XT[e] - X[e], y = GT[e] - G[e];
        d3[0] += s * y; d3[1] += s * s; d3[2] += y * y;
      }
      block_sum<3, REFINE_WAVES>(d3, red);
      const bool keep = d3[0] > CURVATURE_EPS * sqrt(d3[1]) * sqrt(d3[2]);      // else the slot keeps the oldest pair
      for (int e = t; e < nv; e += REFINE_THREADS) {
        if (keep) { S[head * slot + e] = XT[e] - X[e]; Y[head * slot + e] = GT[e] - G[e]; }
        X[e] = XT[e]; G[e] = GT[e];
      }
      E = Et;
      if (keep) {
        if (t == 0) rho[head] = 1.0 / d3[0];
        gamma = d3[0] / d3[2];
        head = (head + 1) % REFINE_HISTORY;
        m = min(m + 1, REFINE_HISTORY);
      }
      __syncthreads();                                         // rho, X and G before anything reads them
    }
    ++stages_done;
  }
  __syncthreads();
  evaluate(X, G, CB, red, n, offsets, entries, last, pr, terms);
  ++evals;
  double gmax = 0.0, cl[1] = {0.0};
  for (int e = t; e < nv; e += REFINE_THREADS) gmax = fmax(gmax, fabs(G[e]));
  gmax = block_max<REFINE_WAVES>(gmax, red);
  for (int i = t; i + 1 < n; i += REFINE_THREADS) {
    const D3 dv = load3<double>(X + 9 * i + 6) - load3<double>(X + 9 * i + 9);
    cl[0] += fabs(sqrt(dot(dv, dv)) - BOND_C_N);
  }
  block_sum<1, REFINE_WAVES>(cl, red);
  double broken[1] = {0.0};
  for (int e = t; e < 9 * L; e += REFINE_THREADS) {
    float v = e < nv ? (float)X[e] : 0.f;
    if (!isfinite(v)) { v = 0.f; broken[0] += 1.0; }
    out[e] = v;
  }
  block_sum<1, REFINE_WAVES>(broken, red);
  if (t == 0) {
    status[b] = st_bits | (broken[0] != 0.0 ? 1 : 0);
    dg[0] = finite_or_zero(e_start);
    dg[1] = finite_or_zero(total_energy(terms, last));
    for (int k = 0; k < 8; ++k) dg[2 + k] = finite_or_zero(terms[k]);
    dg[10] = iters; dg[11] = evals; dg[12] = finite_or_zero(gmax); dg[13] = finite_or_zero(cl[0] / (double)(n - 1));
    dg[14] = stages_done; dg[15] = 0.0;
  }
}

int convert_stage(const double* s6, Stage& st, int L) {
  T2P_REQUIRE(s6[0] >= 0.0 && s6[1] >= 0.0 && s6[5] >= 0.0 && s6[5] <= 100000.0, "refine: a stage needs sep_lo, sep_hi >= 0 and 0 <= max_iter <= 100000");
  T2P_REQUIRE(std::isfinite(s6[2]) && std::isfinite(s6[3]) && std::isfinite(s6[4]) && s6[2] >= 0.0 && s6[3] >= 0.0 && s6[4] >= 0.0,
              "refine: the weights of a stage must be finite and not negative");
  st.sep_lo = (int)std::min(s6[0], (double)(L + 1));
  st.sep_hi = (int)std::min(s6[1], (double)(L + 1));
  st.w_dist = s6[2]; st.w_ang = s6[3]; st.w_rep = s6[4];
  st.max_iter = (int)s6[5];
  return T2P_OK;
}
int convert_params(float dist_std, float angle_std_deg, float arm_min_deg, Params& pr) {
  T2P_REQUIRE(dist_std > 0.f && angle_std_deg > 0.f, "refine: the standard deviations must be positive");
  T2P_REQUIRE(arm_min_deg >= 0.f && arm_min_deg < 90.f, "refine: arm_min lies in [0, 90) degrees");
  pr.inv_dist_std = 1.0 / (double)dist_std;
  pr.inv_angle_std = 1.0 / ((double)angle_std_deg * DEG);
  pr.arm_min = (double)arm_min_deg * DEG;
  return T2P_OK;
}

}  // namespace

long refine_workspace_bytes(int B, int L) {
  if (B <= 0 || L <= 0 || L > REFINE_MAX_L) return -1;
  return (long)RefineWorkspace(B, L).total;
}

int launch_restraint_energy(const float* xyz, const float* absval, const int* lengths, int B, int L, const double* stage6, float dist_std,
                            float angle_std_deg, float arm_min_deg, double* out9, double* grad, void* workspace, long workspace_bytes,
                            hipStream_t s) {
  T2P_REQUIRE(grad, "restraint_energy arguments");
  return launch_restraint_energy_grouped(xyz, absval, lengths, B, 1, L, stage6, dist_std, angle_std_deg, arm_min_deg, out9, grad, workspace,
                                         workspace_bytes, s);
}

// B candidates, each with its own coordinates and length; candidate c reads the maps of chain c / group; grad may be null
int launch_restraint_energy_grouped(const float* xyz, const float* absval, const int* lengths, int B, int group, int L, const double* stage6,
                                    float dist_std, float angle_std_deg, float arm_min_deg, double* out9, double* grad, void* workspace,
                                    long workspace_bytes, hipStream_t s) {
  T2P_REQUIRE(xyz && absval && lengths && stage6 && out9 && workspace && B > 0 && L > 0 && group > 0, "restraint_energy arguments");
  T2P_REQUIRE(L <= REFINE_MAX_L && B <= 65535, "restraint_energy: at most " + std::to_string(REFINE_MAX_L) + " residues and 65535 chains");
  Stage st;
  Params pr;
  T2P_TRY(convert_stage(stage6, st, L));
  T2P_TRY(convert_params(dist_std, angle_std_deg, arm_min_deg, pr));
  const RefineWorkspace ws(B, L);
  T2P_REQUIRE(workspace_bytes >= (long)ws.total, "restraint_energy: workspace smaller than t2p_op_refine_ws(batch, L)");
  char* w = (char*)workspace;
  const int lds = refine_lds_bytes(L);
  auto kernel = group == 1 && grad ? restraint_energy_kernel<false> : restraint_energy_kernel<true>;
  T2P_TRY(ensure_dynamic_lds((const void*)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(B), dim3(REFINE_THREADS), lds, s, xyz, absval, lengths, L, st, pr, out9, grad, (int*)(w + ws.offsets),
                     (Entry*)(w + ws.entries), group);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

int launch_refine_backbone(const float* xyz_in, const float* absval, const int* lengths, int B, int L, const double* schedule, int n_stages,
                           float dist_std, float angle_std_deg, float arm_min_deg, float* xyz_out, int* status, double* diag, void* workspace,
                           long workspace_bytes, hipStream_t s) {
  return launch_refine_grouped(xyz_in, absval, lengths, B, 1, L, schedule, n_stages, dist_std, angle_std_deg, arm_min_deg, xyz_out,
                               status, diag, workspace, workspace_bytes, s);
}

// B candidates, each with its own coordinates and length (one below 2 is how a caller leaves a candidate out: status -1, zeros);
// candidate c reads the maps of chain c / group
int launch_refine_grouped(const float* xyz_in, const float* absval, const int* lengths, int B, int group, int L,
                          const double* schedule, int n_stages, float dist_std, float angle_std_deg, float arm_min_deg, float* xyz_out,
                          int* status, double* diag, void* workspace, long workspace_bytes, hipStream_t s) {
  T2P_REQUIRE(xyz_in && absval && lengths && schedule && xyz_out && status && diag && workspace && B > 0 && L > 0 && group > 0,
              "refine_backbone arguments");
  T2P_REQUIRE(L <= REFINE_MAX_L && B <= 65535, "refine_backbone: at most " + std::to_string(REFINE_MAX_L) + " residues and 65535 chains");
  T2P_REQUIRE(n_stages >= 1 && n_stages <= REFINE_MAX_STAGES, "refine_backbone: 1 to " + std::to_string(REFINE_MAX_STAGES) + " stages");
  Schedule sched;
  Params pr;
  sched.count = n_stages;
  for (int k = 0; k < REFINE_MAX_STAGES; ++k) sched.s[k] = Stage{0, 0, 0, 0.0, 0.0, 0.0};
  for (int k = 0; k < n_stages; ++k) T2P_TRY(convert_stage(schedule + 6 * k, sched.s[k], L));
  T2P_TRY(convert_params(dist_std, angle_std_deg, arm_min_deg, pr));
  const RefineWorkspace ws(B, L);
  T2P_REQUIRE(workspace_bytes >= (long)ws.total, "refine_backbone: workspace smaller than t2p_op_refine_ws(batch, L)");
  char* w = (char*)workspace;
  const int lds = refine_lds_bytes(L);
  auto kernel = group == 1 ? refine_kernel<false> : refine_kernel<true>;
  T2P_TRY(ensure_dynamic_lds((const void*)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(B), dim3(REFINE_THREADS), lds, s, xyz_in, absval, lengths, L, sched, pr, xyz_out, status, diag,
                     (int*)(w + ws.offsets), (Entry*)(w + ws.entries), (double*)(w + ws.history), group);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

}  // namespace t2p
