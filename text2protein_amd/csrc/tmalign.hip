// TM-align on the device: the default path of the reference's tm/TMalign.cpp for a batch of pairs of CA traces.
//
// One workgroup per pair, of 4 wavefronts (3 when La, the padded length of the a chains, exceeds 192: the LDS budget).  Chain a is TM-align's Chain_1
// (x, the one superimposed), chain b its Chain_2 (y).  The program of a workgroup is TMalign_main (TMalign.cpp:3923) with uniform
// control flow; what is parallel is a TASK that one wavefront runs alone from start to end, with no workgroup barrier inside it:
//   threading     one task per shift k of get_initial and of get_initial_fgt's loops: one get_score_fast (three Kabsch fits)
//   get_initial5  one task per (i_frag, i, j): a Kabsch fit of two fragments, a DP, get_score_fast on its alignment
//   search        one task per (L_ini, start) fragment of TMscore8_search: the first fit and up to 20 extension iterations
// Wave w runs the tasks w, w + W, w + 2W, ... of a stage's list in the reference's loop order; a stage ends with one merge through LDS.
// The merge keeps the reference's tie rule -- the first maximum in loop order for TMscore8_search (>) and get_initial5 (>), the last
// for the threading loops (>=) -- by comparing (score, task index), so a pair's result does not depend on the number of wavefronts or
// on which of them ran a task.
//
// Inside a task the 64 lanes split the residues of chain b, at most TM_MAX_L / 64 = 4 per lane (residue j = r * 64 + lane).  An
// alignment is a map b -> a (int16 per residue of b, in LDS); the aligned pairs of a lane sit in registers, the selected subset of a
// fit is a bit mask per lane, the 3x3 covariance and the scores are butterfly sums over the lanes (the same bits in every lane), and
// rotated coordinates are recomputed from (t, u) wherever they are needed.  Kabsch is the reference's closed-form cubic
// (TMalign.cpp:983) statement by statement, with the data-dependent subscripts written as selects so that nothing goes to scratch.
//
// NWDP_TM runs inside one wavefront: lane l owns the columns l C .. l C + C - 1 (C = ceil(len_b / 64)), row i is worked on by lane l
// at step i + l, and the value and path bit of the cell to the left come from lane l - 1 by a cross-lane move.  Score cells are
// computed on the fly from the coordinates and the secondary-structure bytes.  No value or score matrix exists: per cell TWO bits are
// kept in LDS, `path` (the cell came from the diagonal) and `dir` (v >= h, the comparison the reference's traceback repeats on the value
// matrix: TMalign.cpp:1388-1395 reads exactly the h and v the forward pass compared), one byte per (row, lane) = 64 bytes per row and
// wavefront.  The traceback runs on lane 0.
//
// Double throughout; the float32 inputs are widened on load (they are kept as float32 in LDS, which loses nothing).
#include "t2p_common.h"
#include "t2p_kernels.h"
#include "wave_reduce.h"

namespace t2p {
namespace {

constexpr int TM_R = TM_MAX_L / 64;             // residues of chain b per lane
constexpr int TM_SLOT = 16;                     // doubles per wavefront in a merge: score, task, t[3], u[9]
constexpr int TM_NONE_FIRST = 0x7fffffff;       // task index of "no task" where the first maximum wins
constexpr float TM_MAX_COORD = 1.0e6f;           // |coordinate| above this (or not finite): the pair is refused
// Caps of the three relaxation loops.  With usable coordinates they end long before: a cut of 2^20 A^2 / 2048 A exceeds any distance
// inside two superimposed chains of 256 residues (973 A when fully extended), and 1.1^400 x 4.25 A any CA-CA step.  They are a second
// line of defence: whatever reaches the loops, a workgroup ends.
constexpr int TM_CAP_FAST = 1 << 21, TM_CAP_FUN8 = 1 << 12, TM_CAP_FRAG = 400;
constexpr int TM_WS_BYTES = 256;                // the workspace holds the bad-pair flag only

struct TmLayout {                               // byte offsets into the dynamic LDS of one workgroup
  int slots, xa, ya, maps, wmaps, secx, secy, bits, total;
  int La, Lb, W;
  __host__ __device__ TmLayout(int La_, int Lb_, int W_) : La(La_), Lb(Lb_), W(W_) {
    int o = 0;
    auto take = [&](int n) { const int at = o; o += (n + 15) & ~15; return at; };
    slots = take(W * TM_SLOT * 8);
    xa = take(La * 3 * 4);
    ya = take(Lb * 3 * 4);
    maps = take(3 * Lb * 2);                    // M0 (best so far), M1 (this seed / DP_iter's best), M2 (DP_iter's current)
    wmaps = take(2 * W * Lb * 2);               // per wavefront: get_initial5's current and best alignment
    secx = take(La);
    secy = take(Lb);
    bits = take(W * La * 64);                   // per wavefront: path | dir << 4 of the lane's (up to) four columns, per row
    total = o;
  }
};

int tm_waves(int La) { return La <= 192 ? 4 : 3; }        // 64 KB of LDS without opting in: DESIGN.md 8g has the figures

__device__ __forceinline__ int bcount(bool b) { return __popcll(__ballot(b)); }
__device__ __forceinline__ double pick3(int i, double a0, double a1, double a2) { return i == 0 ? a0 : (i == 1 ? a1 : a2); }
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ---- Kabsch (TMalign.cpp:983) from the sums over the selected pairs: s = [sum x | sum y | sum x_a y_b (a major)] ----
// one normalised eigenvector column (the body of the reference's `for l` loop)
__device__ __forceinline__ void eig_col(double d, const double (&rr)[6], double (&col)[3]) {
  const double eps = 0.00000001;
  double ss[6];
  ss[0] = (d - rr[2]) * (d - rr[5]) - rr[4] * rr[4];
  ss[1] = (d - rr[5]) * rr[1] + rr[3] * rr[4];
  ss[2] = (d - rr[0]) * (d - rr[5]) - rr[3] * rr[3];
  ss[3] = (d - rr[2]) * rr[3] + rr[1] * rr[4];
  ss[4] = (d - rr[0]) * rr[4] + rr[1] * rr[3];
  ss[5] = (d - rr[0]) * (d - rr[2]) - rr[1] * rr[1];
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (fabs(ss[k]) <= eps) ss[k] = 0.0;
  int j;
  if (fabs(ss[0]) >= fabs(ss[2])) j = fabs(ss[0]) < fabs(ss[5]) ? 2 : 0;
  else if (fabs(ss[2]) >= fabs(ss[5])) j = 1;
  else j = 2;
  col[0] = pick3(j, ss[0], ss[1], ss[3]);       // ip = {0, 1, 3, 1, 2, 4, 3, 4, 5}
  col[1] = pick3(j, ss[1], ss[2], ss[4]);
  col[2] = pick3(j, ss[3], ss[4], ss[5]);
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) q = q + col[i] * col[i];
  q = q > eps ? 1.0 / sqrt(q) : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) col[i] = col[i] * q;
}

// v (to be made orthonormal to the unit vector w) after `v -= (v . w) w`: the reference's `if (p <= tol) ... else ...`; false = failed
__device__ __forceinline__ bool complete(double (&v)[3], const double (&w)[3], double p) {
  const double tol = 0.01;
  if (p <= tol) {
    int j = 0;
    p = 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (!(p < fabs(w[i]))) { p = fabs(w[i]); j = i; }
    const int k = j == 2 ? 0 : j + 1, l = j == 0 ? 2 : j - 1;          // ip2312 = {1, 2, 0, 1}
    const double wk = pick3(k, w[0], w[1], w[2]), wl = pick3(l, w[0], w[1], w[2]);
    p = sqrt(wk * wk + wl * wl);
    if (!(p > tol)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = i == j ? 0.0 : (i == k ? -wl / p : wk / p);
  } else {
    p = 1.0 / sqrt(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = v[i] * p;
  }
  return true;
}

// mode 1 of the reference: t, u, the rotation of x onto y (u = identity, t = 0 where the reference leaves them so)
__device__ __forceinline__ void kabsch_core(int n, const double (&s)[15], double (&t)[3], double (&u)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) u[i][j] = i == j ? 1.0 : 0.0;
  }
  if (n < 1) return;
  double xc[3], yc[3], r[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { xc[i] = s[i] / n; yc[i] = s[3 + i] / n; }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) r[j][c] = s[6 + 3 * c + j] - s[c] * s[3 + j] / n;
  double det = r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0]) +
               r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]);
  double rr[6];
  rr[0] = r[0][0] * r[0][0] + r[1][0] * r[1][0] + r[2][0] * r[2][0];
  rr[1] = r[0][0] * r[0][1] + r[1][0] * r[1][1] + r[2][0] * r[2][1];
  rr[2] = r[0][1] * r[0][1] + r[1][1] * r[1][1] + r[2][1] * r[2][1];
  rr[3] = r[0][0] * r[0][2] + r[1][0] * r[1][2] + r[2][0] * r[2][2];
  rr[4] = r[0][1] * r[0][2] + r[1][1] * r[1][2] + r[2][1] * r[2][2];
  rr[5] = r[0][2] * r[0][2] + r[1][2] * r[1][2] + r[2][2] * r[2][2];
  const double spur = (rr[0] + rr[2] + rr[5]) / 3.0;
  const double cof = (((((rr[2] * rr[5] - rr[4] * rr[4]) + rr[0] * rr[5]) - rr[3] * rr[3]) + rr[0] * rr[2]) - rr[1] * rr[1]) / 3.0;
  det = det * det;
  double e0 = spur, e1 = spur, e2 = spur;
  double a[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  bool a_failed = false;
  if (spur > 0) {
    double d = spur * spur;
    const double h = d - cof;
    const double g = (spur * cof - det) / 2.0 - spur * h;
    if (h > 0) {
      const double sqrth = sqrt(h);
      d = h * h * h - g * g;
      if (d < 0.0) d = 0.0;
      d = atan2(sqrt(d), -g) / 3.0;
      const double cth = sqrth * cos(d);
      const double sth = sqrth * 1.73205080756888 * sin(d);
      e0 = (spur + cth) + cth;
      e1 = (spur - cth) + sth;
      e2 = (spur - cth) - sth;
      {
        double c0[3], c2[3];
        eig_col(e0, rr, c0);
        eig_col(e2, rr, c2);
        d = c0[0] * c2[0] + c0[1] * c2[1] + c0[2] * c2[2];
        const bool big = (e0 - e1) > (e1 - e2);               // m1 = 2, m = 0; else m1 = 0, m = 2
        double am[3], am1[3];
        double p = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          am[i] = big ? c0[i] : c2[i];
          am1[i] = big ? c2[i] : c0[i];
          am1[i] = am1[i] - d * am[i];
          p = p + am1[i] * am1[i];
        }
        a_failed = !complete(am1, am, p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          a[i][0] = big ? am[i] : am1[i];
          a[i][2] = big ? am1[i] : am[i];
        }
        if (!a_failed) {
          a[0][1] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
          a[1][1] = a[2][2] * a[0][0] - a[2][0] * a[0][2];
          a[2][1] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
        }
      }
    }
    if (!a_failed) {
      double b0[3], b1[3], b2[3];
      double q0 = 0.0, q1 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        b0[i] = r[i][0] * a[0][0] + r[i][1] * a[1][0] + r[i][2] * a[2][0];
        q0 = q0 + b0[i] * b0[i];
        b1[i] = r[i][0] * a[0][1] + r[i][1] * a[1][1] + r[i][2] * a[2][1];
        q1 = q1 + b1[i] * b1[i];
      }
      const double eps = 0.00000001;
      q0 = q0 > eps ? 1.0 / sqrt(q0) : 0.0;
      q1 = q1 > eps ? 1.0 / sqrt(q1) : 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) { b0[i] = b0[i] * q0; b1[i] = b1[i] * q1; }
      d = b0[0] * b1[0] + b0[1] * b1[1] + b0[2] * b1[2];
      double p = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        b1[i] = b1[i] - d * b0[i];
        p += b1[i] * b1[i];
      }
      if (complete(b1, b0, p)) {
        b2[0] = b0[1] * b1[2] - b1[1] * b0[2];
        b2[1] = b0[2] * b1[0] - b1[2] * b0[0];
        b2[2] = b0[0] * b1[1] - b1[0] * b0[1];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) u[i][j] = b0[i] * a[j][0] + b1[i] * a[j][1] + b2[i] * a[j][2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = ((yc[i] - u[i][0] * xc[0]) - u[i][1] * xc[1]) - u[i][2] * xc[2];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = ((yc[i] - u[i][0] * xc[0]) - u[i][1] * xc[1]) - u[i][2] * xc[2];
  }
}

// ---- the aligned pairs of a lane ----
struct Pairs {
  double x[TM_R][3], y[TM_R][3];
  int rank[TM_R];              // position of the pair in the list TM-align builds (in the order of chain b)
  unsigned valid;              // bit r: residue r * 64 + lane of b is aligned
  int n;                       // pairs in the wavefront
};

__device__ __forceinline__ void rot(const double (&t)[3], const double (&u)[3][3], const double (&x)[3], double (&o)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = t[i] + (u[i][0] * x[0] + u[i][1] * x[1] + u[i][2] * x[2]);
}
__device__ __forceinline__ double dist2(const double (&a)[3], const double (&b)[3]) {
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// the pairs (x[ix[r]], y[iy[r]]) for the bits of `valid`; ranks follow the order of r * 64 + lane
__device__ __forceinline__ void gather(Pairs& P, const float* xa, const float* ya, const int (&ix)[TM_R], const int (&iy)[TM_R], unsigned valid, int lane) {
  P.valid = valid;
  int base = 0;
#pragma unroll
  for (int r = 0; r < TM_R; ++r) {
    const bool ok = (valid >> r) & 1u;
    const unsigned long long m = __ballot(ok);
    P.rank[r] = base + __popcll(m & ((1ull << lane) - 1ull));
    base += __popcll(m);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P.x[r][c] = ok ? (double)xa[ix[r] * 3 + c] : 0.0;
      P.y[r][c] = ok ? (double)ya[iy[r] * 3 + c] : 0.0;
    }
  }
  P.n = base;
}

__device__ __forceinline__ void pairs_of_map(Pairs& P, const float* xa, const float* ya, const short* map, int ylen, int lane) {
  int ix[TM_R], iy[TM_R];
  unsigned valid = 0;
#pragma unroll
  for (int r = 0; r < TM_R; ++r) {
    const int j = r * 64 + lane;
    const int i = j < ylen ? (int)map[j] : -1;
    ix[r] = i < 0 ? 0 : i;
    iy[r] = j < ylen ? j : 0;
    if (i >= 0) valid |= 1u << r;
  }
  gather(P, xa, ya, ix, iy, valid, lane);
}

// a gapless threading: residue j of b in [jlo, jhi) is aligned to i = j + s of a when i is in [ilo, ihi)
struct Thread { int jlo, jhi, s, ilo, ihi; };
__device__ __forceinline__ int thread_map(const Thread& th, int j) {
  const int i = j + th.s;
  return (j >= th.jlo && j < th.jhi && i >= th.ilo && i < th.ihi) ? i : -1;
}
__device__ __forceinline__ void pairs_of_thread(Pairs& P, const float* xa, const float* ya, const Thread& th, int ylen, int lane) {
  int ix[TM_R], iy[TM_R];
  unsigned valid = 0;
#pragma unroll
  for (int r = 0; r < TM_R; ++r) {
    const int j = r * 64 + lane;
    const int i = j < ylen ? thread_map(th, j) : -1;
    ix[r] = i < 0 ? 0 : i;
    iy[r] = j < ylen ? j : 0;
    if (i >= 0) valid |= 1u << r;
  }
  gather(P, xa, ya, ix, iy, valid, lane);
}

// Kabsch over the pairs of `sel`
__device__ __forceinline__ void fit(const Pairs& P, unsigned sel, double (&t)[3], double (&u)[3][3]) {
  double s[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) s[k] = 0.0;
  int n = 0;
#pragma unroll
  for (int r = 0; r < TM_R; ++r) {
    const bool on = (sel >> r) & 1u;
    n += bcount(on);
    if (on) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        s[c] += P.x[r][c];
        s[3 + c] += P.y[r][c];
#pragma unroll
        for (int b = 0; b < 3; ++b) s[6 + 3 * c + b] += P.x[r][c] * P.y[r][b];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 15; ++k) s[k] = wave_sum(s[k]);
  kabsch_core(n, s, t, u);
}

// squared distances of the pairs under (t, u) and the sum of 1 / (1 + d / d02) over the pairs with d <= cut (cut < 0: over all)
__device__ __forceinline__ double distances(const Pairs& P, const double (&t)[3], const double (&u)[3][3], double d02, double cut, double (&di)[TM_R]) {
  double sum = 0.0;
#pragma unroll
  for (int r = 0; r < TM_R; ++r) {
    double xr[3];
    rot(t, u, P.x[r], xr);
    di[r] = dist2(xr, P.y[r]);
    if (((P.valid >> r) & 1u) && (cut < 0.0 || di[r] <= cut)) sum += 1.0 / (1.0 + di[r] / d02);
  }
  return wave_sum(sum);
}

// get_score_fast (TMalign.cpp:2194)
__device__ __forceinline__ double score_fast(const Pairs& P, double d02, double d0s) {
  double t[3], u[3][3], di[TM_R];
  const int n = P.n;
  unsigned sel = P.valid;
  double tm = 0.0, best = 0.0;
  const double d002 = d0s * d0s;
  for (int pass = 0; pass < 3; ++pass) {
    fit(P, sel, t, u);
    tm = distances(P, t, u, d02, -1.0, di);
    if (pass == 0 || tm >= best) best = tm;
    if (pass == 2) break;
    double d002t = pass == 0 ? d002 : d002 + 1;
    int cnt;
    for (int relax = 0;; ++relax) {
      sel = 0;
      cnt = 0;
#pragma unroll
      for (int r = 0; r < TM_R; ++r) {
        const bool on = ((P.valid >> r) & 1u) && di[r] <= d002t;
        cnt += bcount(on);
        if (on) sel |= 1u << r;
      }
      if (cnt < 3 && n > 3 && relax < TM_CAP_FAST) d002t += 0.5;
      else break;
    }
    if (pass == 0 && cnt == n) break;
  }
  return best;
}

// one (L_ini, start) fragment of TMscore8_search (TMalign.cpp:1857-1955)
struct Best { double score; int task; double t[3]; double u[3][3]; };

__device__ __forceinline__ void search_task(const Pairs& P, int L, int start, bool m8, double d0s, double norm, double d8sq, double d02, int task, Best& best) {
  const int n = P.n;
  unsigned sel = 0;
#pragma unroll
  for (int r = 0; r < TM_R; ++r)
    if (((P.valid >> r) & 1u) && P.rank[r] >= start && P.rank[r] < start + L) sel |= 1u << r;
  double t[3], u[3][3], di[TM_R];
  for (int it = 0; it <= 20; ++it) {
    const unsigned old = sel;
    fit(P, sel, t, u);
    const double score = distances(P, t, u, d02, m8 ? d8sq : -1.0, di) / norm;
    const double d = it == 0 ? d0s - 1 : d0s + 1;
    double dt = d * d;
    int inc = 0;
    while (true) {                                         // score_fun8's relaxation of the cut
      sel = 0;
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < TM_R; ++r) {
        const bool on = ((P.valid >> r) & 1u) && di[r] < dt;
        cnt += bcount(on);
        if (on) sel |= 1u << r;
      }
      if (cnt < 3 && n > 3 && inc < TM_CAP_FUN8) {
        ++inc;
        const double dinc = d + inc * 0.5;
        dt = dinc * dinc;
      } else break;
    }
    if (score > best.score) {
      best.score = score;
      best.task = task;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        best.t[i] = t[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) best.u[i][j] = u[i][j];
      }
    }
    if (it > 0 && __ballot(sel != old) == 0ull) break;     // i_ali == k_ali
  }
}

struct Ctx {
  const float *xa, *ya;
  const unsigned char *secx, *secy;
  short *M0, *M1, *M2, *wcur, *wbest;
  double* slots;
  unsigned char* bits;
  int xlen, ylen, W, wave, lane, tid, nthreads, bits_stride;
};

// the wavefronts' candidates -> the winner, the same bits in every thread.  last: the highest task index wins a tie, else the lowest
__device__ __forceinline__ void merge(const Ctx& c, Best& b, bool last) {
  double* s = c.slots + c.wave * TM_SLOT;
  if (c.lane == 0) {
    s[0] = b.score;
    s[1] = (double)b.task;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      s[2 + i] = b.t[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) s[5 + 3 * i + j] = b.u[i][j];
    }
  }
  __syncthreads();
  int bw = 0;
  double bs = c.slots[0];
  int bt = (int)c.slots[1];
  for (int w = 1; w < c.W; ++w) {
    const double sc = c.slots[w * TM_SLOT];
    const int tk = (int)c.slots[w * TM_SLOT + 1];
    if (sc > bs || (sc == bs && (last ? tk > bt : tk < bt))) { bw = w; bs = sc; bt = tk; }
  }
  s = c.slots + bw * TM_SLOT;
  b.score = bs;
  b.task = bt;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    b.t[i] = s[2 + i];
#pragma unroll
    for (int j = 0; j < 3; ++j) b.u[i][j] = s[5 + 3 * i + j];
  }
  __syncthreads();
}

// TMscore8_search / TMscore8_search_standard (norm <= 0: by the number of pairs) over the pairs of `map`, by the whole workgroup
__device__ __forceinline__ double search(const Ctx& c, const short* map, int step, bool m8, double d0s, double norm, double d8sq, double d02,
                                         double (&t)[3], double (&u)[3][3]) {
  Pairs P;
  pairs_of_map(P, c.xa, c.ya, map, c.ylen, c.lane);
  const int n = P.n;
  if (norm <= 0.0) norm = (double)n;
  const int lmin = n < 4 ? n : 4;
  Best best;
  best.score = -1.0;
  best.task = TM_NONE_FIRST;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    best.t[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) best.u[i][j] = i == j ? 1.0 : 0.0;
  }
  int g = 0;
  for (int i_init = 0; i_init < 6; ++i_init) {
    int L = i_init == 5 ? lmin : (n >> i_init);
    const bool lastL = i_init == 5 || L <= lmin;
    if (lastL) L = lmin;
    const int imax = n - L;
    const int count = imax == 0 ? 1 : (imax + step - 1) / step + 1;
    for (int k = 0; k < count; ++k, ++g) {
      if (g % c.W != c.wave) continue;
      const int start = k * step < imax ? k * step : imax;
      search_task(P, L, start, m8, d0s, norm, d8sq, d02, g, best);
    }
    if (lastL) break;
  }
  merge(c, best, false);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = best.t[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) u[i][j] = best.u[i][j];
  }
  return best.score;
}

// NWDP_TM by one wavefront.  mode 0: cells 1 / (1 + d / d02) under (t, u); 1: bonus where the secondary structures agree; 2: both.
__device__ __forceinline__ void wave_dp(const Ctx& c, int mode, const double (&t)[3], const double (&u)[3][3], double d02, double gap, double bonus,
                                        short* map) {
  const int xlen = c.xlen, ylen = c.ylen, lane = c.lane;
  unsigned char* bits = c.bits + c.wave * c.bits_stride;
  const int C = (ylen + 63) >> 6;                           // columns per lane, 1 .. 4
  const int j0 = lane * C;
  const int nl = (ylen + C - 1) / C;                        // lanes that own a column
  double yc[TM_R][3];
  unsigned char sy[TM_R];
#pragma unroll
  for (int k = 0; k < TM_R; ++k) {
    const bool on = k < C && j0 + k < ylen;
    const int j = on ? j0 + k : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) yc[k][a] = (double)c.ya[j * 3 + a];
    sy[k] = c.secy[j];
  }
  for (int j = lane; j < ylen; j += 64) map[j] = -1;
  double vprev[TM_R] = {0.0, 0.0, 0.0, 0.0};                // val[i - 1][own columns]
  unsigned pprev = 0;                                       // path[i - 1][own columns]
  double diag_l = 0.0;                                      // val[i - 1][j0 - 1]
  double outv = 0.0;                                        // val / path of the lane's last column in the row it worked on last
  unsigned outp = 0;
  const int steps = xlen + nl - 1;
  for (int s = 0; s < steps; ++s) {
    double lv = __shfl_up(outv, 1, 64);
    unsigned lp = __shfl_up(outp, 1, 64);
    if (lane == 0) { lv = 0.0; lp = 0; }
    const int i = s - lane;                                 // row, 0-based
    if (i >= 0 && i < xlen && lane < nl) {
      double xr[3], xx[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) xr[a] = (double)c.xa[i * 3 + a];
      rot(t, u, xr, xx);
      const unsigned char sx = c.secx[i];
      double left = lv, dg = diag_l;
      unsigned leftp = lp, pb = 0, db = 0;
#pragma unroll
      for (int k = 0; k < TM_R; ++k) {
        if (k < C && j0 + k < ylen) {
          double sc = 0.0;
          if (mode != 1) sc = 1.0 / (1.0 + dist2(xx, yc[k]) / d02);
          if (mode != 0 && sx == sy[k]) sc = sc + bonus;
          const double d = dg + sc;
          const double h = vprev[k] + (((pprev >> k) & 1u) ? gap : 0.0);
          const double v = left + (leftp ? gap : 0.0);
          const bool isd = d >= h && d >= v;
          const bool vh = v >= h;
          const double nv = isd ? d : (vh ? v : h);
          dg = vprev[k];
          vprev[k] = nv;
          left = nv;
          leftp = isd ? 1u : 0u;
          pb |= (isd ? 1u : 0u) << k;
          db |= (vh ? 1u : 0u) << k;
        }
      }
      pprev = pb;
      diag_l = lv;
      outv = left;
      outp = leftp;
      bits[i * 64 + lane] = (unsigned char)(pb | (db << 4));
    }
  }
  wave_fence();
  if (lane == 0) {                                          // the traceback (TMalign.cpp:1376-1397)
    int i = xlen, j = ylen;
    while (i > 0 && j > 0) {
      const int jj = j - 1;
      int l, k;
      if (C == 1) { l = jj; k = 0; }
      else if (C == 2) { l = jj >> 1; k = jj & 1; }
      else if (C == 3) { l = jj / 3; k = jj - 3 * l; }
      else { l = jj >> 2; k = jj & 3; }
      const unsigned b = bits[(i - 1) * 64 + l];
      if ((b >> k) & 1u) { map[jj] = (short)(i - 1); --i; --j; }
      else if ((b >> (4 + k)) & 1u) --j;
      else --i;
    }
  }
  wave_fence();
}

// the shifts of one threading loop: task g in [0, cnt) is the shift k0 + g; s = sbase + k
struct Seg { int cnt, k0, jlo, jhi, sbase, ilo, ihi; };
__device__ __forceinline__ Thread seg_thread(const Seg& a, const Seg& b, int g) {
  const bool first = g < a.cnt;
  const Seg& q = first ? a : b;
  const int k = q.k0 + (first ? g : g - a.cnt);
  return Thread{q.jlo, q.jhi, q.sbase + k, q.ilo, q.ihi};
}

// get_initial / get_initial_fgt: the last maximum of get_score_fast over the shifts of a, then of b; its map goes to `out`
__device__ __forceinline__ void thread_stage(const Ctx& c, const Seg& a, const Seg& b, double d02, double d0s, short* out) {
  Best best;
  best.score = -1.0;
  best.task = -1;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    best.t[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) best.u[i][j] = 0.0;
  }
  const int total = a.cnt + b.cnt;
  for (int g = c.wave; g < total; g += c.W) {
    Pairs P;
    const Thread th = seg_thread(a, b, g);
    pairs_of_thread(P, c.xa, c.ya, th, c.ylen, c.lane);
    const double sc = score_fast(P, d02, d0s);
    if (sc >= best.score) { best.score = sc; best.task = g; }
  }
  merge(c, best, true);
  const Thread th = seg_thread(a, b, best.task < 0 ? 0 : best.task);
  for (int j = c.tid; j < c.ylen; j += c.nthreads) out[j] = (short)thread_map(th, j);
  __syncthreads();
}

// find_max_frag (TMalign.cpp:2678) on a trace in LDS; every thread runs it
__device__ __forceinline__ void find_max_frag(const float* x, int len, int& start_max, int& end_max) {
  const double dcu0 = 4.25;
  int r_min = (int)(len * 1.0 / 3.0);
  if (r_min > 4) r_min = 4;
  int lfr_max = 0, inc = 0;
  double dcu_cut = dcu0 * dcu0;
  start_max = 0;
  end_max = 0;
  while (lfr_max < r_min && inc <= TM_CAP_FRAG) {
    lfr_max = 0;
    int j = 1, start = 0;
    for (int i = 1; i < len; ++i) {
      const double a[3] = {(double)x[(i - 1) * 3], (double)x[(i - 1) * 3 + 1], (double)x[(i - 1) * 3 + 2]};
      const double b[3] = {(double)x[i * 3], (double)x[i * 3 + 1], (double)x[i * 3 + 2]};
      if (dist2(a, b) < dcu_cut) {
        ++j;
        if (i == len - 1) {
          if (j > lfr_max) { lfr_max = j; start_max = start; end_max = i; }
          j = 1;
        }
      } else {
        if (j > lfr_max) { lfr_max = j; start_max = start; end_max = i - 1; }
        j = 1;
        start = i;
      }
    }
    if (lfr_max < r_min) {
      ++inc;
      const double dinc = pow(1.1, (double)inc) * dcu0;
      dcu_cut = dinc * dinc;
    }
  }
}

// the fragment [start, start + L) after get_initial_fgt's trim (TMalign.cpp:2885-2897): applied when L == L0
__device__ __forceinline__ void trim(int& start, int& L, int L0) {
  if (L == L0) {
    const int n1 = (int)(L0 * 0.1), n2 = (int)(L0 * 0.89);
    start += n1;
    L = n2 - n1 + 1;
  }
}
__device__ __forceinline__ int fgt_min_ali(int a, int b) {
  const int m = (int)((a < b ? a : b) / 2.5);
  return m <= 3 ? 3 : m;
}

__device__ __forceinline__ void copy_map(const Ctx& c, short* dst, const short* src) {
  for (int j = c.tid; j < c.ylen; j += c.nthreads) dst[j] = src[j];
  __syncthreads();
}

// a refused pair: zero outputs, a map of -1, status 1 (every thread of the workgroup calls it)
__device__ __forceinline__ void refuse_pair(int p, int Lb, double* out8, int* b2a, double* rot12, int* status) {
  const int tid = threadIdx.x;
  if (tid < 8) out8[(size_t)p * 8 + tid] = 0.0;
  if (rot12 && tid < 12) rot12[(size_t)p * 12 + tid] = 0.0;
  if (b2a)
    for (int j = tid; j < Lb; j += blockDim.x) b2a[(size_t)p * Lb + j] = -1;
  if (tid == 0) status[p] = 1;
}

__global__ __launch_bounds__(256) void tm_align_kernel(const float* __restrict__ xyz_a, const int* __restrict__ len_a, int n_a, int La, int atoms_a,
                                                       const float* __restrict__ xyz_b, const int* __restrict__ len_b, int n_b, int Lb, int atoms_b,
                                                       const int* __restrict__ pairs, double* __restrict__ out8, int* __restrict__ b2a,
                                                       double* __restrict__ rot12, int* __restrict__ status, int* __restrict__ bad_flag) {
  extern __shared__ __align__(16) unsigned char tm_lds[];
  const int p = blockIdx.x, tid = threadIdx.x;
  int ia, ib;
  if (pairs) { ia = pairs[2 * p]; ib = pairs[2 * p + 1]; }
  else { ia = p / n_b; ib = p % n_b; }
  const bool bad = ia < 0 || ia >= n_a || ib < 0 || ib >= n_b;
  const int xlen = bad ? 0 : len_a[ia], ylen = bad ? 0 : len_b[ib];
  if (bad || xlen < 5 || ylen < 5 || xlen > La || ylen > Lb || xlen > TM_MAX_L || ylen > TM_MAX_L) {     // uniform over the workgroup
    refuse_pair(p, Lb, out8, b2a, rot12, status);
    if (bad && tid == 0) *bad_flag = 1;
    return;
  }
  Ctx c;
  c.W = blockDim.x >> 6;
  const TmLayout lay(La, Lb, c.W);
  float* xa = (float*)(tm_lds + lay.xa);
  float* ya = (float*)(tm_lds + lay.ya);
  unsigned char* secx = tm_lds + lay.secx;
  unsigned char* secy = tm_lds + lay.secy;
  c.xa = xa; c.ya = ya; c.secx = secx; c.secy = secy;
  c.slots = (double*)(tm_lds + lay.slots);
  c.M0 = (short*)(tm_lds + lay.maps);
  c.M1 = c.M0 + Lb;
  c.M2 = c.M1 + Lb;
  c.wave = tid >> 6; c.lane = tid & 63; c.tid = tid; c.nthreads = blockDim.x;
  c.wcur = (short*)(tm_lds + lay.wmaps) + (2 * c.wave) * Lb;
  c.wbest = c.wcur + Lb;
  c.bits = tm_lds + lay.bits;
  c.bits_stride = La * 64;
  c.xlen = xlen; c.ylen = ylen;

  // the CA traces, widened where they are used.  A coordinate that is not finite (or beyond TM_MAX_COORD) would turn every distance
  // into NaN, which no cut of the relaxation loops below ever admits: such a pair is refused here, by the whole workgroup at once.
  int usable = 1;
  for (int k = tid; k < xlen * 3; k += blockDim.x) {
    const float v = xyz_a[(((size_t)ia * La + k / 3) * atoms_a + (atoms_a == 3 ? 1 : 0)) * 3 + k % 3];
    if (!(fabsf(v) <= TM_MAX_COORD)) usable = 0;            // false for NaN and Inf as well
    xa[k] = v;
  }
  for (int k = tid; k < ylen * 3; k += blockDim.x) {
    const float v = xyz_b[(((size_t)ib * Lb + k / 3) * atoms_b + (atoms_b == 3 ? 1 : 0)) * 3 + k % 3];
    if (!(fabsf(v) <= TM_MAX_COORD)) usable = 0;
    ya[k] = v;
  }
  if (!__syncthreads_and(usable)) {                         // the same answer in every thread; also the barrier after the loads
    refuse_pair(p, Lb, out8, b2a, rot12, status);
    return;
  }
  // make_sec (TMalign.cpp:2436-2491): 1 coil, 2 helix, 3 turn, 4 strand
  for (int k = tid; k < xlen + ylen; k += blockDim.x) {
    const bool isx = k < xlen;
    const float* q = isx ? xa : ya;
    const int len = isx ? xlen : ylen, i = isx ? k : k - xlen;
    unsigned char sres = 1;
    if (i - 2 >= 0 && i + 2 < len) {
      double r5[5][3];
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int a = 0; a < 3; ++a) r5[m][a] = (double)q[(i - 2 + m) * 3 + a];
      const double d13 = sqrt(dist2(r5[0], r5[2])), d14 = sqrt(dist2(r5[0], r5[3])), d15 = sqrt(dist2(r5[0], r5[4]));
      const double d24 = sqrt(dist2(r5[1], r5[3])), d25 = sqrt(dist2(r5[1], r5[4])), d35 = sqrt(dist2(r5[2], r5[4]));
      if (fabs(d15 - 6.37) < 2.1 && fabs(d14 - 5.18) < 2.1 && fabs(d25 - 5.18) < 2.1 && fabs(d13 - 5.45) < 2.1 && fabs(d24 - 5.45) < 2.1 &&
          fabs(d35 - 5.45) < 2.1)
        sres = 2;
      else if (fabs(d15 - 13) < 1.42 && fabs(d14 - 10.4) < 1.42 && fabs(d25 - 10.4) < 1.42 && fabs(d13 - 6.1) < 1.42 && fabs(d24 - 6.1) < 1.42 &&
               fabs(d35 - 6.1) < 1.42)
        sres = 4;
      else if (d15 < 8) sres = 3;
    }
    (isx ? secx : secy)[i] = sres;
  }
  __syncthreads();

  // parameter_set4search (TMalign.cpp:1647)
  const int minlen = xlen < ylen ? xlen : ylen;
  const double Lnorm = (double)minlen;
  const double d0 = (minlen <= 19 ? 0.168 : 1.24 * pow(Lnorm - 15.0, 1.0 / 3) - 1.8) + 0.8;
  const double D0_MIN = d0;
  double d0s = d0;
  if (d0s > 8) d0s = 8;
  if (d0s < 4.5) d0s = 4.5;
  const double score_d8 = 1.5 * pow(Lnorm, 0.3) + 3.5;
  const double d8sq = score_d8 * score_d8, d02 = d0 * d0;
  const double ddcc = minlen <= 40 ? 0.1 : 0.4;
  double d01 = d0 + 1.5;
  if (d01 < D0_MIN) d01 = D0_MIN;
  const double d012 = d01 * d01;

  double TMmax = -1.0;
  int seed_best = 0;
  double t[3], u[3][3];
  for (int si = 0; si < 5; ++si) {
    short* seed_map = si == 0 ? c.M0 : c.M1;               // get_initial writes the best map itself
    bool have = true;
    if (si == 0 || si == 4) {
      Seg a{0, 0, 0, 0, 0, 0, 0}, b{0, 0, 0, 0, 0, 0, 0};
      if (si == 0) {                                        // get_initial (TMalign.cpp:2341)
        int min_ali = minlen / 2;
        if (min_ali <= 5) min_ali = 5;
        const int n1 = -ylen + min_ali, n2 = xlen - min_ali;
        a = Seg{n2 - n1 + 1, n1, 0, ylen, 0, 0, xlen};
      } else {                                              // get_initial_fgt (TMalign.cpp:2744)
        int xs, xe, ys, ye;
        find_max_frag(xa, xlen, xs, xe);
        find_max_frag(ya, ylen, ys, ye);
        const int Lx = xe - xs + 1, Ly = ye - ys + 1;
        const int Lfr = Lx < Ly ? Lx : Ly;
        const bool use_x = Lx < Ly || (Lx == Ly && xlen <= ylen);
        const bool use_y = Lx > Ly || (Lx == Ly && xlen >= ylen);          // both when Lx == Ly and xlen == ylen
        const int L0 = minlen;
        if (use_x) {
          int st = xs, L1 = Lfr;
          trim(st, L1, L0);
          const int ma = fgt_min_ali(L1, ylen);
          const int n1 = -ylen + ma, n2 = L1 - ma;
          a = Seg{n2 - n1 + 1, n1, 0, ylen, st, st, st + L1};
        }
        if (use_y) {
          int st = ys, L2 = use_x ? Ly : Lfr;
          trim(st, L2, L0);
          const int ma = fgt_min_ali(xlen, L2);
          const int n1 = -L2 + ma, n2 = xlen - ma;
          b = Seg{n2 - n1 + 1, n1, st, st + L2, -st, 0, xlen};
        }
        if (b.cnt < 0) b.cnt = 0;
      }
      if (a.cnt < 0) a.cnt = 0;
      thread_stage(c, a, b, d02, d0s, seed_map);
    } else if (si == 1 || si == 3) {
      if (c.wave == 0) {
        if (si == 1) {                                      // get_initial_ss: DP on the secondary-structure strings, gap -1
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            t[i] = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) u[i][j] = i == j ? 1.0 : 0.0;
          }
          wave_dp(c, 1, t, u, 1.0, -1.0, 1.0, c.M1);
        } else {                                            // get_initial_ssplus (TMalign.cpp:2613-2675) from the best map so far
          Pairs P;
          double ts[3], us[3][3];
          pairs_of_map(P, c.xa, c.ya, c.M0, ylen, c.lane);
          fit(P, P.valid, ts, us);
          wave_dp(c, 2, ts, us, d012, -1.0, 0.5, c.M1);
        }
      }
      __syncthreads();
    } else {                                                // get_initial5 (TMalign.cpp:2514)
      int nj1 = xlen > 250 ? 45 : (xlen > 200 ? 35 : (xlen > 150 ? 25 : 15));
      if (nj1 > xlen / 3) nj1 = xlen / 3;
      int nj2 = ylen > 250 ? 45 : (ylen > 200 ? 35 : (ylen > 150 ? 25 : 15));
      if (nj2 > ylen / 3) nj2 = ylen / 3;
      Best best;
      best.score = 0.0;                                     // GLmax = 0: a candidate must score above it
      best.task = TM_NONE_FIRST;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        best.t[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) best.u[i][j] = 0.0;
      }
      int g = 0;
      for (int i_frag = 0; i_frag < 2; ++i_frag) {
        int nf = i_frag == 0 ? 20 : 100;
        const int cap = i_frag == 0 ? minlen / 3 : minlen / 2;
        if (nf > cap) nf = cap;
        const int m1 = xlen - nf + 1, m2 = ylen - nf + 1;
        for (int i = 0; i < m1; i += nj1)
          for (int j = 0; j < m2; j += nj2, ++g) {
            if (g % c.W != c.wave) continue;
            Pairs P;
            int ix[TM_R], iy[TM_R];
            unsigned valid = 0;
#pragma unroll
            for (int r = 0; r < TM_R; ++r) {
              const int k = r * 64 + c.lane;
              const bool on = k < nf;
              ix[r] = on ? i + k : 0;
              iy[r] = on ? j + k : 0;
              if (on) valid |= 1u << r;
            }
            gather(P, c.xa, c.ya, ix, iy, valid, c.lane);
            double tf[3], uf[3][3];
            fit(P, valid, tf, uf);
            wave_dp(c, 0, tf, uf, d012, 0.0, 0.0, c.wcur);
            pairs_of_map(P, c.xa, c.ya, c.wcur, ylen, c.lane);
            const double gl = score_fast(P, d02, d0s);
            if (gl > best.score) {
              best.score = gl;
              best.task = g;
              for (int q = c.lane; q < ylen; q += 64) c.wbest[q] = c.wcur[q];
              wave_fence();
            }
          }
      }
      merge(c, best, false);
      have = best.task != TM_NONE_FIRST;
      if (have && c.wave == best.task % c.W)
        for (int q = c.lane; q < ylen; q += 64) c.M1[q] = c.wbest[q];
      __syncthreads();
    }
    if (!have) continue;

    // detailed_search on the seed, then DP_iter from its superposition (TMalign.cpp:4033-4219)
    double TM = search(c, seed_map, 40, true, d0s, Lnorm, d8sq, d02, t, u);
    if (TM > TMmax) {
      TMmax = TM;
      seed_best = si;
      if (si != 0) copy_map(c, c.M0, c.M1);
    }
    const bool iterate = si == 0 || TM > TMmax * (si == 1 ? 0.2 : ddcc);
    if (iterate) {
      const int g1 = si == 4 ? 1 : 0, itmax = (si == 2 || si == 4) ? 2 : 30;
      double tm_best = -1.0, tm_old = 0.0;
      for (int g = g1; g < 2; ++g) {
        const double gap = g == 0 ? -0.6 : 0.0;
        for (int it = 0; it < itmax; ++it) {
          if (c.wave == 0) wave_dp(c, 0, t, u, d02, gap, 0.0, c.M2);
          __syncthreads();
          const double tm = search(c, c.M2, 40, true, d0s, Lnorm, d8sq, d02, t, u);
          if (tm > tm_best) {
            tm_best = tm;
            copy_map(c, c.M1, c.M2);
          }
          if (it > 0 && fabs(tm_old - tm) < 0.000001) break;
          tm_old = tm;
        }
      }
      if (tm_best > TMmax) {
        TMmax = tm_best;
        seed_best = si;
        copy_map(c, c.M0, c.M1);
      }
    }
  }

  // the final searches (TMalign.cpp:4333-4409): simplify_step = 1
  search(c, c.M0, 1, true, d0s, 0.0, d8sq, d02, t, u);
  for (int j = tid; j < ylen; j += blockDim.x) {
    const int i = c.M0[j];
    short keep = -1;
    if (i >= 0) {
      const double xr[3] = {(double)xa[i * 3], (double)xa[i * 3 + 1], (double)xa[i * 3 + 2]};
      const double yr[3] = {(double)ya[j * 3], (double)ya[j * 3 + 1], (double)ya[j * 3 + 2]};
      double xt[3];
      rot(t, u, xr, xt);
      if (sqrt(dist2(xt, yr)) <= score_d8) keep = (short)i;
    }
    c.M1[j] = keep;
  }
  __syncthreads();
  // rmsd0 (TMalign.cpp:4381): the least RMSD of the kept pairs.  The reference takes it from Kabsch mode 0 as e0 - 2 (sum of the singular
  // values), which cancels to ~1e-7 A of noise when the chains coincide; the same minimum is formed here as the residual under the
  // optimal rotation, which does not cancel.
  double rmsd0;
  int n_ali8;
  {
    Pairs P;
    pairs_of_map(P, c.xa, c.ya, c.M1, ylen, c.lane);
    n_ali8 = P.n;
#pragma unroll
    for (int r = 0; r < TM_R; ++r) {
      double xt[3];
      rot(t, u, P.x[r], xt);
#pragma unroll
      for (int a = 0; a < 3; ++a) P.x[r][a] = ((P.valid >> r) & 1u) ? xt[a] : 0.0;
    }
    double tz[3], uz[3][3];
    fit(P, P.valid, tz, uz);
    double e = 0.0;
#pragma unroll
    for (int r = 0; r < TM_R; ++r) {
      double xt[3];
      rot(tz, uz, P.x[r], xt);
      if ((P.valid >> r) & 1u) e += dist2(xt, P.y[r]);
    }
    e = wave_sum(e);
    rmsd0 = n_ali8 > 0 ? sqrt(e / n_ali8) : 0.0;
  }
  // parameter_set4final (TMalign.cpp:1687) for len_b (TM-align's TM1, whose superposition it prints) and for len_a (TM2)
  double tm_ab[2], d0_ab[2], t0[3], u0[3][3];
  for (int w = 0; w < 2; ++w) {
    const double Lf = w == 0 ? (double)ylen : (double)xlen;
    double d0f = Lf <= 21 ? 0.5 : 1.24 * pow(Lf - 15.0, 1.0 / 3) - 1.8;
    if (d0f < 0.5) d0f = 0.5;
    double d0sf = d0f;
    if (d0sf > 8) d0sf = 8;
    if (d0sf < 4.5) d0sf = 4.5;
    d0_ab[w] = d0f;
    if (w == 0) tm_ab[0] = search(c, c.M1, 1, false, d0sf, Lf, d8sq, d0f * d0f, t0, u0);
    else tm_ab[1] = search(c, c.M1, 1, false, d0sf, Lf, d8sq, d0f * d0f, t, u);
  }
  if (tid == 0) {
    double* o = out8 + (size_t)p * 8;
    o[0] = tm_ab[1];
    o[1] = tm_ab[0];
    o[2] = rmsd0;
    o[3] = (double)n_ali8;
    o[4] = d0_ab[1];
    o[5] = d0_ab[0];
    o[6] = TMmax;
    o[7] = (double)seed_best;
    status[p] = 0;
    if (rot12) {
      double* q = rot12 + (size_t)p * 12;
      for (int i = 0; i < 3; ++i) {
        q[i] = t0[i];
        for (int j = 0; j < 3; ++j) q[3 + 3 * i + j] = u0[i][j];
      }
    }
  }
  if (b2a)
    for (int j = tid; j < Lb; j += blockDim.x) b2a[(size_t)p * Lb + j] = j < ylen ? (int)c.M1[j] : -1;
}

}  // namespace

long tm_align_workspace_bytes(int n_pairs, int La, int Lb) {
  if (n_pairs <= 0 || La <= 0 || Lb <= 0 || La > TM_MAX_L || Lb > TM_MAX_L) return -1;
  return TM_WS_BYTES;
}

int tm_align_info(int La, int Lb, int* out4) {
  T2P_REQUIRE(out4 && La > 0 && Lb > 0 && La <= TM_MAX_L && Lb <= TM_MAX_L, "tm_align_info arguments");
  hipFuncAttributes attr;
  T2P_HIP_CHECK(hipFuncGetAttributes(&attr, (const void*)tm_align_kernel));
  out4[0] = tm_waves(La);
  out4[1] = TmLayout(La, Lb, tm_waves(La)).total;
  out4[2] = attr.numRegs;
  out4[3] = (int)attr.localSizeBytes;
  return T2P_OK;
}

int launch_tm_align(const float* xyz_a, const int* len_a, int n_a, int La, int atoms_a, const float* xyz_b, const int* len_b, int n_b, int Lb,
                    int atoms_b, const int* pairs, int n_pairs, double* out8, int* b2a, double* rot12, int* status, void* workspace,
                    long workspace_bytes, hipStream_t s) {
  T2P_REQUIRE(xyz_a && len_a && xyz_b && len_b && out8 && status && workspace, "tm_align: a required pointer is null");
  T2P_REQUIRE(n_a > 0 && n_b > 0 && La > 0 && Lb > 0 && n_pairs > 0, "tm_align: the chain counts, padded lengths and pair count must be positive");
  T2P_REQUIRE(atoms_a == 1 || atoms_a == 3, "tm_align: atoms_a must be 1 (a CA trace) or 3 (N / CA / C), not " + std::to_string(atoms_a));
  T2P_REQUIRE(atoms_b == 1 || atoms_b == 3, "tm_align: atoms_b must be 1 (a CA trace) or 3 (N / CA / C), not " + std::to_string(atoms_b));
  T2P_REQUIRE(La <= TM_MAX_L && Lb <= TM_MAX_L, "tm_align: at most " + std::to_string(TM_MAX_L) + " residues per chain");
  T2P_REQUIRE(pairs || (long)n_a * n_b == (long)n_pairs, "tm_align: without a pair list n_pairs must be n_a * n_b");
  T2P_REQUIRE(workspace_bytes >= tm_align_workspace_bytes(n_pairs, La, Lb), "tm_align: workspace smaller than t2p_op_tm_align_ws(n_pairs, La, Lb)");
  const int W = tm_waves(La);
  const int lds = TmLayout(La, Lb, W).total;
  T2P_REQUIRE(lds <= 65536, "tm_align: LDS layout above 64 KB");
  T2P_HIP_CHECK(hipMemsetAsync(workspace, 0, sizeof(int), s));
  hipLaunchKernelGGL(tm_align_kernel, dim3(n_pairs), dim3(64 * W), lds, s, xyz_a, len_a, n_a, La, atoms_a, xyz_b, len_b, n_b, Lb, atoms_b, pairs,
                     out8, b2a, rot12, status, (int*)workspace);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

}  // namespace t2p
