// Refinement in rounds: the reference's "diversify backbone" move on N / CA / C chains held in Cartesian coordinates, and
// its loop over runs -- perturb the best structure so far, minimise with the run's weights, keep the result when it scores lower
// (rosetta_min/run.py:88-151) -- without a host round trip.
//
// The move.  Atoms a_0 .. a_3n-1 run N, CA, C per residue.  For k >= 3, b_k = |a_k - a_k-1|, theta_k the angle at a_k-1 and
// tau_k = dihedral(a_k-3, a_k-2, a_k-1, a_k), measured in double from the fp32 input by one thread per atom.  tau_3i+2 (it places C_i:
// phi_i) takes + dphi_i for i >= 1, tau_3i+3 (it places N_i+1: psi_i) + dpsi_i for i <= n - 2; omega, bonds and angles stay as
// measured.  Atoms 0..2 are copied; every later atom is placed from the three rebuilt atoms before it (NeRF), sequentially, by one lane
// per candidate: 3 n placements of one sincos and some sixty flops each.  Nothing is reduced across lanes, so two calls give the same
// bits, and a chain's move depends on (seed, stream, chain id, its own coordinates) only.
//
// The frame of a placement is bc = (c - b) / |c - b|, nrm = (b - a) x bc normalised, m = nrm x bc, and
//   d = c + b_k (-cos theta bc + sin theta (cos tau m + sin tau nrm)).
// Fallback, where the frame is undefined: bc = (1, 0, 0) when |c - b|^2 < GUARD; nrm = bc x e, e the coordinate axis on which bc is
// shortest, when |(b - a) x bc|^2 < GUARD (a, b, c collinear).  sin theta enters as a factor only, never as a denominator, so a straight
// angle needs no case of its own.  Outputs are always finite.
//
// The loop.  Per round r: perturb_kernel (incumbent -> replicas candidates, stream_base + 16 r; round 0 keeps candidate 0 as the input),
// refine_kernel over batch x replicas workgroups (refine.hip, candidate c with the maps of chain c / replicas and its own length, -1 for
// a candidate the move refused), restraint_energy_kernel
// under the selection stage on what the minimiser wrote, select_kernel (lowest E_sel among status 0 / 1, ties to the lowest index; it
// replaces the incumbent when strictly lower).  The incumbent lives in the caller's xyz_out / status / diag.
#include <cmath>

#include "backbone_geom.h"
#include "philox.h"
#include "t2p_common.h"
#include "t2p_kernels.h"

namespace t2p {
namespace {

constexpr int PERTURB_THREADS = 256;
using namespace geom;        // D3, GUARD, DEG, angle, dihedral_guarded: the minimiser's own definitions (backbone_geom.h)

__device__ __forceinline__ D3 place(D3 a, D3 b, D3 c, double bond, double cs_theta, double sn_theta, double tau) {
  D3 bc = c - b;
  const double l2 = dot(bc, bc);
  bc = l2 >= GUARD ? (1.0 / sqrt(l2)) * bc : D3{1.0, 0.0, 0.0};
  D3 nrm = cross(b - a, bc);
  double n2 = dot(nrm, nrm);
  if (!(n2 >= GUARD)) {
    const double ax = fabs(bc.x), ay = fabs(bc.y), az = fabs(bc.z);
    const D3 e = (ax <= ay && ax <= az) ? D3{1.0, 0.0, 0.0} : (ay <= az ? D3{0.0, 1.0, 0.0} : D3{0.0, 0.0, 1.0});
    nrm = cross(bc, e);
    n2 = dot(nrm, nrm);
  }
  nrm = (1.0 / sqrt(n2)) * nrm;
  const D3 m = cross(nrm, bc);
  double sn, cs;
  sincos(tau, &sn, &cs);
  return c + bond * ((-cs_theta) * bc + sn_theta * (cs * m + sn * nrm));
}

// One workgroup per chain.  in_status (may be null): a chain whose entry is neither 0 nor 1 has no incumbent and keeps that status.
__global__ __launch_bounds__(PERTURB_THREADS) void perturb_kernel(const float* __restrict__ xyz_in, const int* __restrict__ lengths,
                                                                  const int* __restrict__ chain_ids, const int* __restrict__ in_status, int L,
                                                                  int K, double amp, unsigned long long seed, unsigned long long stream,
                                                                  int keep_first, float* __restrict__ xyz_out, int* __restrict__ status,
                                                                  int* __restrict__ cand_lengths) {
  extern __shared__ double lds[];                               // bond, cos theta, sin theta, tau: 3 L doubles each
  double* bond = lds;
  double* cth = bond + 3 * L;
  double* sth = cth + 3 * L;
  double* tau = sth + 3 * L;
  __shared__ int bad_count;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = lengths[b];
  const float* in = xyz_in + (long)b * L * 9;
  float* out = xyz_out + (long)b * K * L * 9;
  int st = (n >= 2 && n <= L) ? 0 : -1;
  if (st == 0 && in_status != nullptr && in_status[b] != 0 && in_status[b] != 1) st = in_status[b];
  if (t == 0) bad_count = 0;
  __syncthreads();
  if (st == 0) {
    int bad = 0;
    for (int e = t; e < 9 * n; e += PERTURB_THREADS) bad += !isfinite(in[e]);
    if (bad) atomicAdd(&bad_count, bad);                        // an integer count: the order does not matter
  }
  __syncthreads();
  if (st == 0 && bad_count != 0) st = 2;
  if (st != 0) {                                                // uniform over the workgroup
    for (long e = t; e < (long)K * L * 9; e += PERTURB_THREADS) out[e] = 0.f;
    for (int k = t; k < K; k += PERTURB_THREADS) {
      status[b * K + k] = st;
      if (cand_lengths) cand_lengths[b * K + k] = -1;
    }
    return;
  }
  const int na = 3 * n;
  for (int k = 3 + t; k < na; k += PERTURB_THREADS) {
    const D3 p0 = load3<double>(in + 3 * (k - 3)), p1 = load3<double>(in + 3 * (k - 2)), p2 = load3<double>(in + 3 * (k - 1)), p3 = load3<double>(in + 3 * k);
    const double theta = angle(p1, p2, p3);
    const D3 w = p3 - p2;
    bond[k] = sqrt(dot(w, w));
    sincos(theta, &sth[k], &cth[k]);
    tau[k] = dihedral_guarded(p0, p1, p2, p3);
  }
  // the tail past the chain, the first three atoms, and candidate 0 when it is the input itself
  for (long e = t; e < (long)K * L * 9; e += PERTURB_THREADS) {
    const int k = (int)(e / (L * 9)), r = (int)(e - (long)k * L * 9);
    if (r >= 9 * n) out[e] = 0.f;
    else if (r < 9 || (k == 0 && keep_first)) out[e] = in[r];
  }
  for (int k = t; k < K; k += PERTURB_THREADS) {
    status[b * K + k] = 0;
    if (cand_lengths) cand_lengths[b * K + k] = n;
  }
  __syncthreads();
  if (t >= K || (t == 0 && keep_first)) return;
  // one lane per candidate: the sequential rebuild
  const unsigned long long st_k = stream + (unsigned long long)t;
  const long id_hi = (long)((unsigned long long)(uint32_t)(chain_ids ? chain_ids[b] : b) << 32);
  float* o = out + (long)t * L * 9;
  D3 a = load3<double>(in), bb = load3<double>(in + 3), c = load3<double>(in + 6);
  uint32_t w[4];
  philox_counter_training(w, id_hi, st_k);                      // residue 0: its psi moves N_1
  philox4x32_10(w, seed);
  double dpsi = amp * (2.0 * (double)philox_uniform24(w[1]) - 1.0);
  for (int k = 3; k < na; ++k) {
    const int i = k / 3, which = k - 3 * i;
    double delta = 0.0;
    if (which == 0) delta = dpsi;                               // N_i: psi of residue i - 1
    else if (which == 2) {                                      // C_i: phi of residue i; its psi is kept for N_i+1
      philox_counter_training(w, id_hi | (long)i, st_k);
      philox4x32_10(w, seed);
      delta = amp * (2.0 * (double)philox_uniform24(w[0]) - 1.0);
      dpsi = amp * (2.0 * (double)philox_uniform24(w[1]) - 1.0);
    }
    const D3 d = place(a, bb, c, bond[k], cth[k], sth[k], tau[k] + delta * DEG);
    float fx = (float)d.x, fy = (float)d.y, fz = (float)d.z;
    o[3 * k] = isfinite(fx) ? fx : 0.f; o[3 * k + 1] = isfinite(fy) ? fy : 0.f; o[3 * k + 2] = isfinite(fz) ? fz : 0.f;
    a = bb; bb = c; c = d;
  }
}

// One workgroup per chain: the lowest E_sel among the round's valid candidates replaces the incumbent when it is strictly lower.
__global__ __launch_bounds__(64) void select_kernel(const float* __restrict__ cand_xyz, const int* __restrict__ move_status,
                                                    const int* __restrict__ cand_status, const double* __restrict__ cand_diag,
                                                    const double* __restrict__ esel9, int L, int K, int round, int rounds,
                                                    double* __restrict__ e_inc, float* __restrict__ xyz_out, int* __restrict__ status,
                                                    double* __restrict__ diag, double* __restrict__ trace) {
  __shared__ int chosen;
  const int b = blockIdx.x, t = threadIdx.x;
  if (t == 0) {
    int best = -1;
    double e_best = 0.0;
    for (int k = 0; k < K; ++k) {
      const int c = b * K + k, st = move_status[c] != 0 ? move_status[c] : cand_status[c];
      const bool valid = st == 0 || st == 1;
      const double e = valid ? esel9[(long)c * 9 + 8] : 0.0;
      double* tr = trace + (((long)b * rounds + round) * K + k) * 4;
      tr[0] = e; tr[1] = (double)st; tr[2] = cand_diag[(long)c * 16 + 11]; tr[3] = 0.0;
      if (valid && (best < 0 || e < e_best)) { best = k; e_best = e; }
    }
    const bool lower = best >= 0 && (round == 0 || e_best < e_inc[b]);
    if (lower) {
      e_inc[b] = e_best;
      status[b] = cand_status[b * K + best];
      trace[(((long)b * rounds + round) * K + best) * 4 + 3] = 1.0;
    } else if (round == 0) {                                    // no incumbent: the status t2p_op_refine_backbone gives the input
      e_inc[b] = INFINITY;
      status[b] = move_status[b * K] != 0 ? move_status[b * K] : cand_status[b * K];
    }
    chosen = lower ? best : -1;
  }
  __syncthreads();
  const int k = chosen;
  if (k >= 0) {
    const float* src = cand_xyz + (long)(b * K + k) * L * 9;
    for (int e = t; e < 9 * L; e += 64) xyz_out[(long)b * L * 9 + e] = src[e];
    if (t < 16) diag[(long)b * 16 + t] = cand_diag[(long)(b * K + k) * 16 + t];
  } else if (round == 0) {
    for (int e = t; e < 9 * L; e += 64) xyz_out[(long)b * L * 9 + e] = 0.f;
    if (t < 16) diag[(long)b * 16 + t] = 0.0;
  }
}

struct RoundsWorkspace {          // byte offsets into the caller's workspace (WorkspaceCarve)
  size_t moved, refined, move_status, cand_lengths, cand_status, cand_diag, esel, e_inc, refine, total;
  long refine_bytes;
  RoundsWorkspace(int B, int L, int K) {
    WorkspaceCarve w;
    const size_t C = (size_t)B * K;
    moved = w.take(C * L * 9 * 4);
    refined = w.take(C * L * 9 * 4);
    move_status = w.take(C * 4);
    cand_lengths = w.take(C * 4);
    cand_status = w.take(C * 4);
    cand_diag = w.take(C * 16 * 8);
    esel = w.take(C * 9 * 8);
    e_inc = w.take((size_t)B * 8);
    refine_bytes = refine_workspace_bytes((int)C, L);
    refine = w.take((size_t)refine_bytes);
    total = w.total;
  }
};

bool rounds_shape_ok(long B, int L, int K) {
  return B > 0 && L > 0 && L <= REFINE_MAX_L && K >= 1 && K <= REFINE_MAX_REPLICAS && B * K <= 65535;
}

}  // namespace

int launch_perturb_torsions(const float* xyz_in, const int* lengths, const int* chain_ids, const int* in_status, int B, int L, int replicas,
                            float amp_deg, unsigned long long seed, unsigned long long stream, int keep_first, float* xyz_out, int* status,
                            int* cand_lengths, hipStream_t s) {
  T2P_REQUIRE(xyz_in && lengths && xyz_out && status && B > 0 && L > 0, "perturb_torsions arguments");
  T2P_REQUIRE(L <= REFINE_MAX_L && B <= 65535, "perturb_torsions: at most " + std::to_string(REFINE_MAX_L) + " residues and 65535 chains");
  T2P_REQUIRE(replicas >= 1 && replicas <= REFINE_MAX_REPLICAS, "perturb_torsions: 1 to " + std::to_string(REFINE_MAX_REPLICAS) + " replicas");
  T2P_REQUIRE(std::isfinite(amp_deg) && amp_deg >= 0.f, "perturb_torsions: the amplitude (degrees) must be finite and not negative");
  hipLaunchKernelGGL(perturb_kernel, dim3(B), dim3(PERTURB_THREADS), (size_t)4 * 3 * L * 8, s, xyz_in, lengths, chain_ids, in_status, L, replicas,
                     (double)amp_deg, seed, stream, keep_first, xyz_out, status, cand_lengths);
  T2P_HIP_CHECK(hipGetLastError());
  return T2P_OK;
}

long refine_rounds_workspace_bytes(int B, int L, int replicas) {
  if (!rounds_shape_ok(B, L, replicas)) return -1;
  return (long)RoundsWorkspace(B, L, replicas).total;
}

int launch_refine_rounds(const float* xyz_in, const float* absval, const int* lengths, const int* chain_ids, int B, int L,
                         const double* schedules, int rounds, int n_stages, int replicas, const double* select_stage, float amp_deg,
                         unsigned long long seed, unsigned long long stream_base, float dist_std, float angle_std_deg, float arm_min_deg,
                         float* xyz_out, int* status, double* diag, double* trace, void* workspace, long workspace_bytes, hipStream_t s) {
  T2P_REQUIRE(xyz_in && absval && lengths && schedules && select_stage && xyz_out && status && diag && trace && workspace,
              "refine_rounds arguments");
  T2P_REQUIRE(rounds >= 1 && rounds <= REFINE_MAX_ROUNDS, "refine_rounds: 1 to " + std::to_string(REFINE_MAX_ROUNDS) + " rounds");
  T2P_REQUIRE(rounds_shape_ok(B, L, replicas), "refine_rounds: at most " + std::to_string(REFINE_MAX_L) + " residues, 1 to " +
                                                   std::to_string(REFINE_MAX_REPLICAS) + " replicas, batch x replicas <= 65535");
  T2P_REQUIRE(n_stages >= 1 && n_stages <= REFINE_MAX_STAGES, "refine_rounds: 1 to " + std::to_string(REFINE_MAX_STAGES) + " stages");
  const RoundsWorkspace ws(B, L, replicas);
  T2P_REQUIRE(workspace_bytes >= (long)ws.total, "refine_rounds: workspace smaller than t2p_op_refine_rounds_ws(batch, L, replicas)");
  char* w = (char*)workspace;
  float* moved = (float*)(w + ws.moved);
  float* refined = (float*)(w + ws.refined);
  int* move_status = (int*)(w + ws.move_status);
  int* cand_lengths = (int*)(w + ws.cand_lengths);
  int* cand_status = (int*)(w + ws.cand_status);
  double* cand_diag = (double*)(w + ws.cand_diag);
  double* esel = (double*)(w + ws.esel);
  const int C = B * replicas;
  for (int r = 0; r < rounds; ++r) {
    T2P_TRY(launch_perturb_torsions(r == 0 ? xyz_in : xyz_out, lengths, chain_ids, r == 0 ? nullptr : status, B, L, replicas, amp_deg, seed,
                                    stream_base + (unsigned long long)REFINE_STREAM_STRIDE * r, r == 0, moved, move_status, cand_lengths, s));
    T2P_TRY(launch_refine_grouped(moved, absval, cand_lengths, C, replicas, L, schedules + (long)r * n_stages * 6, n_stages, dist_std,
                                  angle_std_deg, arm_min_deg, refined, cand_status, cand_diag, w + ws.refine, ws.refine_bytes, s));
    T2P_TRY(launch_restraint_energy_grouped(refined, absval, cand_lengths, C, replicas, L, select_stage, dist_std, angle_std_deg, arm_min_deg, esel,
                                            nullptr, w + ws.refine, ws.refine_bytes, s));
    hipLaunchKernelGGL(select_kernel, dim3(B), dim3(64), 0, s, refined, move_status, cand_status, cand_diag, esel, L, replicas, r, rounds,
                       (double*)(w + ws.e_inc), xyz_out, status, diag, trace);
    T2P_HIP_CHECK(hipGetLastError());
  }
  return T2P_OK;
}

}  // namespace t2p
