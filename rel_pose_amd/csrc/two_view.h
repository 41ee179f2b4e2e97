// two_view.h -- the two-view geometry primitives of the solver libraries (csrc_eightpoint, csrc_refine, csrc_consensus, csrc_fivepoint,
// csrc_homography, csrc_triangulate), one definition each: the Sampson distance, quaternion <-> rotation, [a]x R, cross / dot,
// unit<N>, the sign rule and the finite check, the Hartley transform of a minimal sample, the null vector of an 8 x 9 matrix and the
// damped Cholesky step of the Levenberg-Marquardt kernels.
//
// Every function is per-thread arithmetic on registers: no LDS, no barrier, every loop unrolled and every index static (nothing goes to
// scratch).  The expression forms -- the order of the sums, the parentheses, the constants -- are part of the libraries' contract (the
// public headers under include/ state them, tests/_*_ref.py restate them): the same inputs give the same bits in every library.
#pragma once
#include "common.h"

constexpr float RP_FINITE = 3.0e38f;                 // |v| <= RP_FINITE: v is a number
constexpr float RP_MIN_SCALE = 1e-30f;               // a mean distance or a norm below this counts as 0

// Sampson distance of x1 <-> x2 under e (row-major), as rel_pose_amd/readout.py: sampson_distance; 0 where the denominator is 0
RP_DEV float sampson(const float (&e)[9], float2 a, float2 b) {
  const float l2x = e[0] * a.x + e[1] * a.y + e[2], l2y = e[3] * a.x + e[4] * a.y + e[5], l2z = e[6] * a.x + e[7] * a.y + e[8];
  const float l1x = e[0] * b.x + e[3] * b.y + e[6], l1y = e[1] * b.x + e[4] * b.y + e[7];
  const float r = b.x * l2x + b.y * l2y + l2z;
  const float den = l2x * l2x + l2y * l2y + l1x * l1x + l1y * l1y;
  return den > 0.f ? r * r / den : 0.f;
}

// v / |v| with the largest magnitude taken out first (no overflow, no underflow); returns |v| (0, or a NaN, for a v that has no direction)
template <int N>
RP_DEV float unit(const float (&v)[N], float (&u)[N]) {
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
    ss += u[i] * u[i];
  }
  const float s = sqrtf(ss);
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = u[i] / s;
  return m * s;
}

RP_DEV void quat_to_rot(const float (&q)[4], float (&R)[9]) {
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - z * w);       R[2] = 2.f * (x * z + y * w);
  R[3] = 2.f * (x * y + z * w);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - x * w);
  R[6] = 2.f * (x * z - y * w);       R[7] = 2.f * (y * z + x * w);       R[8] = 1.f - 2.f * (x * x + y * y);
}

// the unit quaternion (xyzw, w >= 0) of a near-rotation R (row-major), Shepperd's branches; the normalisation re-orthonormalises R
RP_DEV void rot_to_quat(const float (&R)[9], float (&q)[4]) {
  const float tr = R[0] + R[4] + R[8];
  float v[4];
  if (tr > 0.f) {
    v[3] = 1.f + tr; v[0] = R[7] - R[5]; v[1] = R[2] - R[6]; v[2] = R[3] - R[1];
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    v[0] = 1.f + R[0] - R[4] - R[8]; v[3] = R[7] - R[5]; v[1] = R[1] + R[3]; v[2] = R[2] + R[6];
  } else if (R[4] >= R[8]) {
    v[1] = 1.f + R[4] - R[0] - R[8]; v[3] = R[2] - R[6]; v[0] = R[1] + R[3]; v[2] = R[5] + R[7];
  } else {
    v[2] = 1.f + R[8] - R[0] - R[4]; v[3] = R[3] - R[1]; v[0] = R[2] + R[6]; v[1] = R[5] + R[7];
  }
  const float nrm = sqrtf(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
  const float s = v[3] < 0.f ? -1.f : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = nrm > 0.f ? s * v[i] / nrm : (i == 3 ? 1.f : 0.f);
}

// [a]x R, row-major
RP_DEV void cross_times(const float (&a)[3], const float (&R)[9], float (&e)[9]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e[c] = a[1] * R[6 + c] - a[2] * R[3 + c];
    e[3 + c] = a[2] * R[c] - a[0] * R[6 + c];
    e[6 + c] = a[0] * R[3 + c] - a[1] * R[c];
  }
}

RP_DEV void cross(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

RP_DEV float dot(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// every entry is a number
RP_DEV bool all_finite(const float (&m)[9]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && fabsf(m[i]) <= RP_FINITE;
  return ok;
}

// the sign rule of rp_eight_point: the entry of largest magnitude, the first of equal ones, is positive
RP_DEV void sign_rule(float (&m)[9]) {
  float big = fabsf(m[0]), lead = m[0];
#pragma unroll
  for (int i = 1; i < 9; ++i) {
    if (fabsf(m[i]) > big) { big = fabsf(m[i]); lead = m[i]; }
  }
  if (lead < 0.f) {
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = -m[i];
  }
}

// Hartley transform of N points with unit weights about the pivot p[0]: centroid (cx, cy), scale s; false on a breakdown
template <int N>
RP_DEV bool normalise(const float2 (&p)[N], float& cx, float& cy, float& s) {
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    sx += p[k].x - p[0].x;
    sy += p[k].y - p[0].y;
  }
  cx = p[0].x + sx / (float)N;
  cy = p[0].y + sy / (float)N;
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float dx = p[k].x - cx, dy = p[k].y - cy;
    m += sqrtf(dx * dx + dy * dy);
  }
  m = m / (float)N;
  if (!(m >= RP_MIN_SCALE)) return false;
  s = sqrtf(2.f) / m;
  return true;
}

// the null vector f of the 8 x 9 matrix whose rows are m.a[0] .. m.a[7] (a[j] is the j-th COLUMN of the 9 x 8 transpose).
// Householder QR of the transpose, column by column: H_j = I - beta_j v_j v_j^T zeroes column j below its diagonal; v_j stays in
// A[j][j ..].  A zero column gets beta = 0, v = 0: no reflection.  f is the last column of Q = H_0 .. H_7.
// The matrix comes BY VALUE, in a struct: the reflections overwrite it, and with the copy being the function's own the compiler packs
// and contracts the unrolled arithmetic exactly as it does for a matrix declared in place (through a reference into the caller's
// frame it pairs the operations differently, and low-order bits of the result move).
struct Mat8x9 {
  float a[8][9];
};
RP_DEV void null_vector_8x9(Mat8x9 m, float (&f)[9]) {
  float (&A)[8][9] = m.a;
  float beta[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float sig = 0.f;
#pragma unroll
    for (int i = j; i < 9; ++i) sig += A[j][i] * A[j][i];
    const float nrm = sqrtf(sig);
    const float den = sig + fabsf(A[j][j]) * nrm;
    beta[j] = den > 0.f ? 1.f / den : 0.f;
    A[j][j] += copysignf(nrm, A[j][j]);
#pragma unroll
    for (int k = j + 1; k < 8; ++k) {
      float t = 0.f;
#pragma unroll
      for (int i = j; i < 9; ++i) t += A[j][i] * A[k][i];
      t *= beta[j];
#pragma unroll
      for (int i = j; i < 9; ++i) A[k][i] -= t * A[j][i];
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) f[i] = i == 8 ? 1.f : 0.f;
#pragma unroll
  for (int j = 7; j >= 0; --j) {
    float t = 0.f;
#pragma unroll
    for (int i = j; i < 9; ++i) t += A[j][i] * f[i];
    t *= beta[j];
#pragma unroll
    for (int i = j; i < 9; ++i) f[i] -= t * A[j][i];
  }
}

// the Levenberg-Marquardt step (H + lam diag H) delta = -g in the diagonally scaled form by Cholesky; false on a breakdown.
// a: the N (N + 1) / 2 upper entries of H row by row, then the N of g.
template <int N>
RP_DEV bool lm_cholesky_solve(const float (&a)[N * (N + 1) / 2 + N], float lam, float (&delta)[N]) {
  float H[N][N], sc[N], rhs[N];
  int k = 0;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) H[i][j] = H[j][i] = a[k++];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ok = ok && H[i][i] > 0.f && H[i][i] <= RP_FINITE;
    sc[i] = 1.f / sqrtf(H[i][i]);
    rhs[i] = a[N * (N + 1) / 2 + i] * sc[i];
  }
  if (!ok) return false;
  float L[N][N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float p = 1.f + lam;
#pragma unroll
    for (int m = 0; m < j; ++m) p = p - L[j][m] * L[j][m];
    if (!(p > 0.f) || !(p <= RP_FINITE)) return false;
    L[j][j] = sqrtf(p);
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      float v = H[i][j] * sc[i] * sc[j];
#pragma unroll
      for (int m = 0; m < j; ++m) v = v - L[i][m] * L[j][m];
      L[i][j] = v / L[j][j];
    }
  }
  float y[N], z[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float v = rhs[i];
#pragma unroll
    for (int m = 0; m < i; ++m) v = v - L[i][m] * y[m];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    float v = y[i];
#pragma unroll
    for (int m = i + 1; m < N; ++m) v = v - L[m][i] * z[m];
    z[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    delta[i] = -(z[i] * sc[i]);
    ok = ok && fabsf(delta[i]) <= RP_FINITE;
  }
  return ok;
}
