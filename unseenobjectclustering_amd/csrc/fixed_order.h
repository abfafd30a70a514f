// Fixed-order fp64 reductions, order-preserving integer keys and the small eigen-solver shared by the per-object
// statistics (objects.hip) and the support plane (plane.hip).  Everything here returns the same bits from run to run.
#pragma once
#include "common.h"

#include <math.h>

namespace uoc {

__device__ __forceinline__ unsigned long long dkey(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ddecode(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// ---- fixed-order wave64 reductions: one DPP tree per 16-lane row, then rows 0..3 combined in order ----
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = dpp_i<CTRL>((int)b), hi = dpp_i<CTRL>((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// All 64 lanes must be active.  Returns the same bits in every lane and from run to run.
__device__ __forceinline__ double wave_sum_d(double v) {
  v += dpp_d<0xB1>(v);
  v += dpp_d<0x4E>(v);
  v += dpp_d<0x141>(v);
  v += dpp_d<0x140>(v);
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ double wave_max_d(double v) {
  v = fmax(v, dpp_d<0xB1>(v));
  v = fmax(v, dpp_d<0x4E>(v));
  v = fmax(v, dpp_d<0x141>(v));
  v = fmax(v, dpp_d<0x140>(v));
  return fmax(fmax(readlane_d(v, 0), readlane_d(v, 16)), fmax(readlane_d(v, 32), readlane_d(v, 48)));
}

// Cyclic Jacobi on a symmetric 3x3 in fp64: a becomes diagonal, the columns of v the eigenvectors.
__device__ inline void jacobi3(double a[3][3], double v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    const double dia = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
    if (off <= 1e-18 * dia || off == 0.0) break;
    for (int r = 0; r < 3; ++r) {
      const int p = P[r], q = Q[r];
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cth = 1.0 / sqrt(t * t + 1.0), sth = t * cth;
      for (int k = 0; k < 3; ++k) {
        const double akp = a[k][p], akq = a[k][q];
        a[k][p] = cth * akp - sth * akq;
        a[k][q] = sth * akp + cth * akq;
      }
      for (int k = 0; k < 3; ++k) {
        const double apk = a[p][k], aqk = a[q][k];
        a[p][k] = cth * apk - sth * aqk;
        a[q][k] = sth * apk + cth * aqk;
      }
      a[p][q] = a[q][p] = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = cth * vkp - sth * vkq;
        v[k][q] = sth * vkp + cth * vkq;
      }
    }
  }
}

// Descending eigenvalues of a diagonalised 3x3 with their vectors as rows of vec; ties keep the lower index first (a
// 3-element stable sort, unrolled).
__device__ inline void sort_eig3(const double a[3][3], const double v[3][3], double lam[3], double vec[3][3]) {
  for (int i = 0; i < 3; ++i) {
    lam[i] = a[i][i];
    for (int k = 0; k < 3; ++k) vec[i][k] = v[k][i];
  }
  auto swap_if = [&](int i, int j) {  // i < j: move j in front of i when strictly larger
    if (lam[j] > lam[i]) {
      const double t = lam[i];
      lam[i] = lam[j];
      lam[j] = t;
      for (int k = 0; k < 3; ++k) {
        const double u = vec[i][k];
        vec[i][k] = vec[j][k];
        vec[j][k] = u;
      }
    }
  };
  swap_if(1, 2);
  swap_if(0, 1);
  swap_if(1, 2);
}

// Flip e so that its component of largest magnitude is positive (ties: lowest index).
__device__ __forceinline__ void sign_rule(double e[3]) {
  int k = 0;
  for (int i = 1; i < 3; ++i)
    if (fabs(e[i]) > fabs(e[k])) k = i;
  if (e[k] < 0.0)
    for (int i = 0; i < 3; ++i) e[i] = -e[i];
}

}  // namespace uoc
