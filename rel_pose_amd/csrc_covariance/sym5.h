// sym5.h -- the per-thread 5 x 5 algebra of rp_pose_covariance (include/relpose_covariance.h states every step), and the exactly
// restatable frame of the pose.  csrc/two_view.h has the damped Cholesky SOLVE of the Levenberg-Marquardt kernels; what the covariance
// needs beyond it -- the pivots, the inverse, the sandwich product, the Jacobi eigen-decomposition -- lives here, beside its one user.
//
// Everything is arithmetic on registers: no LDS, no barrier, every loop unrolled and every index static (nothing goes to scratch); the
// one rolled loop, over the Jacobi sweeps, has a body whose indices are all static.
#pragma once
#include "../csrc/common.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_covariance.h"

constexpr float COV_PIVOT_MIN = 1e-6f;               // a pivot of the scaled A that is not above this: not determined

// v / |v| with the largest magnitude taken out first, as unit<3> / unit<4> of csrc/two_view.h, but without fused multiply-adds: the
// header promises a frame that numpy float32 restates bit for bit.  Returns |v| (0, or a NaN, for a v that has no direction).
template <int N>
RP_DEV float unit_exact(const float (&v)[N], float (&u)[N]) {
#pragma clang fp contract(off)
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) m = fmaxf(m, fabsf(v[i]));
  if (!(m > 0.f)) {
#pragma unroll
    for (int i = 0; i < N; ++i) u[i] = v[i];
    return 0.f;
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    u[i] = v[i] / m;
    ss = ss + u[i] * u[i];
  }
  const float s = sqrtf(ss);
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = u[i] / s;
  return m * s;
}

// the basis of the tangent plane at the unit vector t by the rule of relpose_refine.h, without fused multiply-adds
RP_DEV void tangent_basis_exact(const float (&t)[3], float (&b1)[3], float (&b2)[3]) {
#pragma clang fp contract(off)
  const float a0 = fabsf(t[0]), a1 = fabsf(t[1]), a2 = fabsf(t[2]);
  int k = a1 < a0 ? 1 : 0;
  k = a2 < (k ? a1 : a0) ? 2 : k;
  float c[3];
  c[0] = k == 0 ? 0.f : k == 1 ? t[2] : -t[1];
  c[1] = k == 0 ? -t[2] : k == 1 ? 0.f : t[0];
  c[2] = k == 0 ? t[1] : k == 1 ? -t[0] : 0.f;
  const float s = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) b1[i] = c[i] / s;
  b2[0] = t[1] * b1[2] - t[2] * b1[1];
  b2[1] = t[2] * b1[0] - t[0] * b1[2];
  b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// C = A^-1 B A^-1 in the diagonally scaled form (steps 1 - 5 of the header).  a: the 15 upper entries of A row by row, then the 15 of B.
// Returns true with C (exactly symmetric) and rho = the smallest pivot; false with rho = the offending pivot (0 for a bad diagonal).
RP_DEV bool sandwich5(const float (&a)[30], float (&C)[5][5], float& rho) {
  float A[5][5], B[5][5], d[5];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = i; j < 5; ++j) {
      A[i][j] = A[j][i] = a[k];
      B[i][j] = B[j][i] = a[15 + k];
      ++k;
    }
  rho = 0.f;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    ok = ok && A[i][i] > 0.f && A[i][i] <= RP_FINITE;
    d[i] = 1.f / sqrtf(A[i][i]);
  }
  if (!ok) return false;
  float L[5][5];
  float low = 1.f;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    float p = 1.f;
#pragma unroll
    for (int m = 0; m < j; ++m) p = p - L[j][m] * L[j][m];
    if (!(p > COV_PIVOT_MIN)) {
      rho = fabsf(p) <= RP_FINITE ? p : 0.f;
      return false;
    }
    low = fminf(low, p);
    L[j][j] = sqrtf(p);
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      float v = A[i][j] * d[i] * d[j];
#pragma unroll
      for (int m = 0; m < j; ++m) v = v - L[i][m] * L[j][m];
      L[i][j] = v / L[j][j];
    }
  }
  rho = low;
  float M[5][5];
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    float y[5], z[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      float v = i == c ? 1.f : 0.f;
#pragma unroll
      for (int m = 0; m < i; ++m) v = v - L[i][m] * y[m];
      y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {
      float v = y[i];
#pragma unroll
      for (int m = i + 1; m < 5; ++m) v = v - L[m][i] * z[m];
      z[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) M[i][c] = z[i];
  }
  float T[5][5];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int l = 0; l < 5; ++l) {
      float v = 0.f;
#pragma unroll
      for (int m = 0; m < 5; ++m) v += M[i][m] * (B[m][l] * d[m] * d[l]);
      T[i][l] = v;
    }
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = i; j < 5; ++j) {
      float v = 0.f;
#pragma unroll
      for (int l = 0; l < 5; ++l) v += T[i][l] * M[j][l];
      v = (d[i] * v) * d[j];
      ok = ok && fabsf(v) <= RP_FINITE;
      C[i][j] = C[j][i] = v;
    }
  return ok;
}

// eigenvalues (descending) of the symmetric C by cyclic Jacobi, RP_COVARIANCE_SWEEPS sweeps, and the eigenvector of the largest one with
// its component of largest magnitude made positive
RP_DEV void jacobi5(const float (&C)[5][5], float (&eig)[5], float (&weak)[5]) {
  float a[5][5], V[5][5];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      a[i][j] = C[i][j];
      V[i][j] = i == j ? 1.f : 0.f;
    }
#pragma unroll 1
  for (int sweep = 0; sweep < RP_COVARIANCE_SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = p + 1; q < 5; ++q) {
        const float apq = a[p][q];
        float t = 0.f;
        if (apq != 0.f) {
          const float theta = (a[q][q] - a[p][p]) / (2.f * apq);
          t = (theta >= 0.f ? 1.f : -1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
        }
        const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = a[q][p] = 0.f;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
          if (r != p && r != q) {
            const float x = a[r][p], y = a[r][q];
            a[r][p] = a[p][r] = c * x - s * y;
            a[r][q] = a[q][r] = s * x + c * y;
          }
          const float x = V[r][p], y = V[r][q];
          V[r][p] = c * x - s * y;
          V[r][q] = s * x + c * y;
        }
      }
  }
  // the eigenvector of the largest diagonal entry, the lowest index on ties
  float big = a[0][0];
#pragma unroll
  for (int r = 0; r < 5; ++r) weak[r] = V[r][0];
#pragma unroll
  for (int i = 1; i < 5; ++i) {
    if (a[i][i] > big) {
      big = a[i][i];
#pragma unroll
      for (int r = 0; r < 5; ++r) weak[r] = V[r][i];
    }
  }
  float lead = weak[0], mag = fabsf(weak[0]);
#pragma unroll
  for (int r = 1; r < 5; ++r) {
    if (fabsf(weak[r]) > mag) { mag = fabsf(weak[r]); lead = weak[r]; }
  }
  if (lead < 0.f) {
#pragma unroll
    for (int r = 0; r < 5; ++r) weak[r] = -weak[r];
  }
  // descending order: a bubble network over static indices
#pragma unroll
  for (int i = 0; i < 5; ++i) eig[i] = a[i][i];
#pragma unroll
  for (int pass = 0; pass < 4; ++pass)
#pragma unroll
    for (int i = 0; i < 4 - pass; ++i) {
      const float hi = fmaxf(eig[i], eig[i + 1]), lo = fminf(eig[i], eig[i + 1]);
      eig[i] = hi;
      eig[i + 1] = lo;
    }
}
