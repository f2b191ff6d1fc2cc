// Device helpers shared by the evaluation translation units (eval.hip, fscore.hip): the fp64 similarity solve, the
// fixed-tree reductions and the fp64 CSR regression.  Everything is __forceinline__: each unit gets its own copy.
#pragma once
#include "p2m_common.h"

namespace p2m {

// ---- the 3x3 similarity solve (Horn's quaternion form) ------------------------------------------------------------
// H = (A - cA)^T (B - cB) / N.  The rotation R (A -> B) maximising tr(R H) is the unit quaternion of the largest
// eigenvalue lam of Horn's symmetric 4x4 matrix built from H; lam = s1 + s2 + sign(det H) s3 - the reference's sum(s)
// after its reflection fix (coord_utils.py:133-137), so c = lam / varP, t = cB - c R cA.  The eigenproblem is solved by
// cyclic Jacobi over the six (p, q) pairs in a fixed order: every index is a compile-time constant (no scratch), and
// every lane that calls it with the same H gets bitwise the same result.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
  if (!(fabs(apq) > 1e-18 * (fabs(app) + fabs(aqq)))) {   // negligible (or zero / NaN): drop it, no rotation
    a[P][Q] = a[Q][P] = 0.0;
    return;
  }
  const double th = (aqq - app) / (2.0 * apq);
  double t;
  if (fabs(th) > 1e150) t = 0.5 / th;
  else t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {                          // a J
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq;
    a[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {                          // J^T (a J)
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk;
    a[Q][k] = s * apk + c * aqk;
  }
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {                          // v J
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}

// H: row-major 3x3 (H[3 i + j] = sum (a_i - cA_i)(b_j - cB_j) / N); varP: population variance of A summed over axes.
// Out: R row-major (A2 = c R a + t), c, t.  varP == 0 (all points of A coincide): c and t are non-finite, as the
// reference's 1 / varP makes them; nothing faults.
__device__ __forceinline__ void similarity_solve(const double* __restrict__ H, double varP, const double* __restrict__ cA,
                                              const double* __restrict__ cB, double* __restrict__ R, double* __restrict__ c_out,
                                              double* __restrict__ t) {
  const double xx = H[0], xy = H[1], xz = H[2], yx = H[3], yy = H[4], yz = H[5], zx = H[6], zy = H[7], zz = H[8];
  double a[4][4] = {{xx + yy + zz, yz - zy, zx - xz, xy - yx},
                    {yz - zy, xx - yy - zz, xy + yx, zx + xz},
                    {zx - xz, xy + yx, -xx + yy - zz, yz + zy},
                    {xy - yx, zx + xz, yz + zy, -xx - yy + zz}};
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 12; sweep++) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] + a[1][3] * a[1][3] +
                       a[2][3] * a[2][3];
    const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
    if (!(off > 1e-36 * dia)) break;                     // converged (quadratically: ~5 sweeps), or all zero / NaN
    jacobi_rot<0, 1>(a, v);
    jacobi_rot<0, 2>(a, v);
    jacobi_rot<0, 3>(a, v);
    jacobi_rot<1, 2>(a, v);
    jacobi_rot<1, 3>(a, v);
    jacobi_rot<2, 3>(a, v);
  }
  // largest eigenvalue and its eigenvector (column of v), selected without a runtime index
  double lam = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
  for (int k = 1; k < 4; k++) {
    if (a[k][k] > lam) {
      lam = a[k][k];
      q0 = v[0][k]; q1 = v[1][k]; q2 = v[2][k]; q3 = v[3][k];
    }
  }
  const double qn = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  q0 *= qn; q1 *= qn; q2 *= qn; q3 *= qn;
  R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3;
  R[1] = 2.0 * (q1 * q2 - q0 * q3);
  R[2] = 2.0 * (q1 * q3 + q0 * q2);
  R[3] = 2.0 * (q1 * q2 + q0 * q3);
  R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
  R[5] = 2.0 * (q2 * q3 - q0 * q1);
  R[6] = 2.0 * (q1 * q3 - q0 * q2);
  R[7] = 2.0 * (q2 * q3 + q0 * q1);
  R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
  const double c = lam / varP;
  *c_out = c;
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = cB[i] - c * (R[3 * i] * cA[0] + R[3 * i + 1] * cA[1] + R[3 * i + 2] * cA[2]);
}

// ---- reductions: fixed trees, every participating lane ends with bitwise the same totals -------------------------------
// xor butterfly over the 64 lanes of a wave (a + b == b + a in IEEE: all lanes agree bitwise)
template <int K>
__device__ __forceinline__ void wave_sum(double (&x)[K]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; k++) x[k] += __shfl_xor(x[k], o);
  }
}
// whole block (NT threads): waves, then the NT / 64 wave totals in wave order.  sh: >= (NT / 64) * K doubles.
template <int NT, int K>
__device__ __forceinline__ void block_sum(double (&x)[K], double* sh) {
  wave_sum<K>(x);
  if (NT == 64) return;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[w * K + k] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double s = sh[k];
    for (int i = 1; i < NT / 64; i++) s += sh[i * K + k];
    x[k] = s;
  }
  __syncthreads();                                       // sh is reused by the next reduction
}

__device__ __forceinline__ double dist3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// regressed joint j, coordinate k, of mesh m (scaled by s, minus `sub`), fp64 over the CSR row
__device__ __forceinline__ double regress(const int* ptr, const int* idx, const float* val, const float* m, float s, int j, int k,
                                          double sub) {
  double acc = 0.0;
  for (int e = ptr[j]; e < ptr[j + 1]; e++) acc += (double)val[e] * ((double)m[idx[e] * 3 + k] * (double)s - sub);
  return acc;
}

}  // namespace p2m
