// Backbone geometry of the structure operators: the one place it is written.
//
// 3-vectors in float or double, the featuriser's virtual Cb, the ideal backbone, angles and the two dihedral forms.  fold.hip,
// refine.hip, refine_rounds.hip, sse.hip and the 6D encode in kernels.hip promise "the same bits whatever the batch, the padding or
// the call" and "the composed loop equals its parts bit for bit"; that holds because they share these definitions, operand order
// included.  Every function is a device-side, always-inlined leaf; the constants are usable on the host as well.
#pragma once
#include <hip/hip_runtime.h>

namespace t2p {
namespace geom {

constexpr double PI = 3.14159265358979323846, DEG = 0.017453292519943295, RAD = 57.29577951308232;      // pi / 180, 180 / pi
constexpr double GUARD = 1e-12;          // floor of every denominator

// The featuriser's virtual Cb: Cb - CA = K1 (b x c) + K2 b + K3 c with b = CA - N, c = C - CA (dataset.py:409).
constexpr double K1 = -0.58273431, K2 = 0.56802827, K3 = -0.54067466;
// Ideal backbone: |b| = 1.458, |c| = 1.525, |C - N'| = 1.329, angle N-CA-C = 111.0 deg, so b . c = -|b||c| cos(111 deg) = 0.796813
// and |b x c| = |b||c| sin(111 deg) = 2.075769.  b x c is orthogonal to b and c, hence
//   |Cb - CA|^2 = K1^2 |b x c|^2 + K2^2 |b|^2 + K3^2 |c|^2 + 2 K2 K3 (b . c)
//              = 1.463186 + 0.685891 + 0.679848 - 0.489432 = 2.339492          ->  R_CB = 1.529540 A
//   cos(N-CA-Cb) = (-b) . (Cb - CA) / (|b| R_CB) = -(K2 |b|^2 + K3 (b . c)) / (|b| R_CB) = -0.776677 / 2.230069 = -0.348275
//                                                                              ->  N-CA-Cb = 110.3818 deg, sin = 0.937392
constexpr double BOND_N_CA = 1.458, BOND_CA_C = 1.525, BOND_C_N = 1.329, ANGLE_N_CA_C = 111.0;           // A, degrees
constexpr double R_CB = 1.529540, COS_NCACB = -0.348275, SIN_NCACB = 0.937392;

// The float twins are the doubles rounded once; each equals the float literal the fp32 kernels were written with.
constexpr float K1_F = (float)K1, K2_F = (float)K2, K3_F = (float)K3;
static_assert(K1_F == -0.58273431f && K2_F == 0.56802827f && K3_F == -0.54067466f, "virtual Cb: float constants");
constexpr float BOND_N_CA_F = (float)BOND_N_CA, BOND_C_N_F = (float)BOND_C_N;
static_assert(BOND_N_CA_F == 1.458f && BOND_C_N_F == 1.329f, "ideal bonds: float constants");
constexpr float R_CB_F = (float)R_CB, COS_NCACB_F = (float)COS_NCACB, SIN_NCACB_F = (float)SIN_NCACB;
static_assert(R_CB_F == 1.529540f && COS_NCACB_F == -0.348275f && SIN_NCACB_F == 0.937392f, "Cb placement: float constants");

template <typename T> struct V3 { T x, y, z; };
using D3 = V3<double>;
using F3 = V3<float>;
template <typename T> struct scalar_of { using type = T; };              // keeps the scalar of s * v out of template deduction
template <typename T> __device__ __forceinline__ V3<T> operator+(V3<T> a, V3<T> b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename T> __device__ __forceinline__ V3<T> operator-(V3<T> a, V3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T> __device__ __forceinline__ V3<T> operator-(V3<T> a) { return {-a.x, -a.y, -a.z}; }
template <typename T> __device__ __forceinline__ V3<T> operator*(typename scalar_of<T>::type s, V3<T> a) { return {s * a.x, s * a.y, s * a.z}; }
template <typename T> __device__ __forceinline__ T dot(V3<T> a, V3<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <typename T> __device__ __forceinline__ V3<T> cross(V3<T> a, V3<T> b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename T> __device__ __forceinline__ void axpy(V3<T>& acc, typename scalar_of<T>::type s, V3<T> a) {
  acc.x += s * a.x; acc.y += s * a.y; acc.z += s * a.z;
}
// three consecutive values, widened (or kept) to the wanted precision: load3<double>(float_ptr)
template <typename T> __device__ __forceinline__ V3<T> load3(const float* p) { return {(T)p[0], (T)p[1], (T)p[2]}; }
template <typename T> __device__ __forceinline__ V3<T> load3(const double* p) { return {(T)p[0], (T)p[1], (T)p[2]}; }
template <typename T> __device__ __forceinline__ void store3(T* p, V3<T> a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

// Cb - CA from b = CA - N and c = C - CA, and the virtual Cb itself
template <typename T> __device__ __forceinline__ V3<T> cb_offset(V3<T> b, V3<T> c) { return (T)K1 * cross(b, c) + (T)K2 * b + (T)K3 * c; }
template <typename T> __device__ __forceinline__ V3<T> virtual_cb(V3<T> n, V3<T> ca, V3<T> c) { return ca + cb_offset(ca - n, c - ca); }

__device__ __forceinline__ double wrap_angle(double x) { return x - 2.0 * PI * rint(x / (2.0 * PI)); }      // into [-pi, pi]

// angle at pb, in [0, pi]; 0 / 0 (a zero arm) is 0.  The long form hands back the arms v = pa - pb and w = pc - pb, v x w and its
// length, which a gradient needs (refine.hip's angle_grad).
__device__ __forceinline__ double angle(D3 pa, D3 pb, D3 pc, D3& v, D3& w, D3& cr, double& sn) {
  v = pa - pb; w = pc - pb; cr = cross(v, w);
  sn = sqrt(dot(cr, cr));
  const double cs = dot(v, w);
  return (sn == 0.0 && cs == 0.0) ? 0.0 : atan2(sn, cs);
}
__device__ __forceinline__ double angle(D3 pa, D3 pb, D3 pc) {
  D3 v, w, cr;
  double sn;
  return angle(pa, pb, pc, v, w, cr, sn);
}

// Dihedral p0-p1-p2-p3, cross-product form: atan2 of ((h x g) x (f x g)) . g / |g| and (f x g) . (h x g), with |g|^2 floored by GUARD, so
// a zero axis gives a finite value and never a NaN.  The text of the minimiser's energy: it is the value of refine.hip's
// dihedral_grad, which calls it, and the measurement of refine_rounds.hip's perturb_kernel -- so the move and the minimiser agree bit
// for bit on every torsion.
__device__ __forceinline__ double dihedral_guarded(D3 p0, D3 p1, D3 p2, D3 p3) {
  const D3 f = p0 - p1, g = p1 - p2, h = p3 - p2;
  const D3 a = cross(f, g), b = cross(h, g);
  const double gl = sqrt(fmax(dot(g, g), GUARD));
  const double y = dot(cross(b, a), g) / gl, x = dot(a, b);
  return (x == 0.0 && y == 0.0) ? 0.0 : atan2(y, x);
}

// Dihedral from its three bond vectors b0 = a - b, b1 = c - b, b2 = d - c, projection form: get_dihedrals (dataset.py:364-380).  A
// zero axis is the reference's NaN -> nan_to_num -> 0, and a zero-length projection leaves x = y = 0 with signs that depend on the other
// vector (atan2(+-0, -0) is +-pi): the angle is undefined there and 0 is returned, whatever the signs of the zeros.  The same sign as
// dihedral_guarded.  Used by the 6D encode (kernels.hip, float, from short differences) and by the restraint score (fold.hip, double).
template <typename T> __device__ __forceinline__ T dihedral_or_zero(V3<T> b0, V3<T> b1, V3<T> b2) {
  const T l = sqrt(dot(b1, b1));
  if (!(l > (T)0)) return (T)0;
  b1 = ((T)1 / l) * b1;
  const V3<T> v = b0 - dot(b0, b1) * b1, w = b2 - dot(b2, b1) * b1;
  const T y = dot(cross(b1, v), w), x = dot(v, w);
  return (x == (T)0 && y == (T)0) ? (T)0 : atan2(y, x);
}
template <typename T> __device__ __forceinline__ T dihedral_or_zero(V3<T> a, V3<T> b, V3<T> c, V3<T> d) {
  const V3<T> b0 = a - b, b2 = d - c;
  return dihedral_or_zero(b0, c - b, b2);
}

}  // namespace geom
}  // namespace t2p
